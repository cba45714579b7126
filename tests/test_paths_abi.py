"""Path batches (vk_paths_*, additive symbols of ABI 7) on the CPU: the eight functions and the compaction hook declared, exported by both
libraries, bound, declared in the Rust shim; the two structs' sizes and offsets as gcc lays them out against the ctypes mirror; no
stream-taking function; the refusals that need no device; the kernel constants the tests' sizes are chosen around; the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import paths_ref
from vecchio_amd import build, ffi
from vecchio_amd.scene import PATH_STATE_DTYPE, RAY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_paths_create", "vk_paths_begin", "vk_paths_step", "vk_paths_read", "vk_paths_cull", "vk_paths_results", "vk_paths_get_info",
             "vk_paths_destroy"]
STRUCTS = {"vk_paths_info": ffi.PathsInfo, "vk_paths_step_info": ffi.PathsStepInfo}


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
    assert re.search(r"\bint vk_debug_compact_paths\s*\(", code(header("vecchio_amd_debug.h")))
    assert re.search(r"\bint vk_debug_paths_last_ms\s*\(", code(header("vecchio_amd_debug.h")))
    for path in (ffi.device_lib_path(), build.build_device_debug()):
        lib = C.CDLL(path)
        for fn in FUNCTIONS + ["vk_debug_compact_paths", "vk_debug_paths_last_ms"]:
            assert hasattr(lib, fn), (path, fn)
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    assert lib.vk_paths_create.argtypes == [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    assert lib.vk_paths_begin.argtypes == [C.c_void_p, C.POINTER(ffi.ShadeParams), C.c_void_p, C.c_void_p, C.c_uint64]
    assert lib.vk_paths_step.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(ffi.PathsStepInfo)]
    assert lib.vk_paths_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.PathsInfo)]
    assert lib.vk_paths_destroy.restype is None and lib.vk_paths_step.restype is C.c_int
    assert len(lib.vk_debug_compact_paths.argtypes) == 11
    assert (ffi.VK_PATHS_LIVE, ffi.VK_PATHS_CULLED) == (1, 4) and ffi.VK_PATHS_LIVE == ffi.VK_SHADE_SCATTERED
    assert re.search(r"VK_PATHS_LIVE = 1 /\* == VK_SHADE_SCATTERED \*/, VK_PATHS_CULLED = 4", hdr)
    # vk_shade_hits' comment now points to the path batch for media
    shade = hdr[hdr.index("shade queries"):hdr.index("typedef struct vk_path_state")]
    assert "A path batch (vk_paths_*, below) traces on the path's stream" in shade


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_paths_create": r"scene: \*mut vk_scene, capacity: u64, out: \*mut \*mut vk_paths\) -> c_int;",
        "vk_paths_begin": r"p: \*mut vk_paths, params: \*const vk_shade_params, rays: \*const vk_ray, states: \*const vk_path_state, n: u64\) -> c_int;",
        "vk_paths_step": r"p: \*mut vk_paths, max_bounces: u32, info: \*mut vk_paths_step_info\) -> c_int;",
        "vk_paths_read": r"p: \*mut vk_paths, ids: \*mut u32, rays: \*mut vk_ray, states: \*mut vk_path_state\) -> c_int;",
        "vk_paths_cull": r"p: \*mut vk_paths, keep: \*const u8, scale: \*const f32\) -> c_int;",
        "vk_paths_results": r"p: \*mut vk_paths, states: \*mut vk_path_state, status: \*mut u32\) -> c_int;",
        "vk_paths_get_info": r"p: \*mut vk_paths, out: \*mut vk_paths_info\) -> c_int;",
        "vk_paths_destroy": r"p: \*mut vk_paths\);",
    }
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_paths \{ _private: \[u8; 0\] \}", rs)
    fields = {
        "vk_paths_info": "pub capacity: u64, pub started: u64, pub live: u64, pub retired: [u64; 5], pub bounces: u32, pub _pad: u32",
        "vk_paths_step_info": "pub traced: u64, pub live: u64, pub missed: u64, pub ended: u64, pub bad: u64, pub bounces: u32, "
                              "pub kernel_launches: u32, pub kernel_ms: f64, pub seconds: f64",
    }
    for name, f in fields.items():
        m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct " + name + r"\s*\{(.*?)\}", rs, flags=re.S)
        assert m and " ".join(m.group(1).split()) == f, name
    for k, v in (("VK_PATHS_LIVE", 1), ("VK_PATHS_CULLED", 4)):
        assert re.search(rf"pub const {k}: u32 = {v};", rs), k


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """vk_paths_info 72 bytes, vk_paths_step_info 64, and every field's offset and size: the header through gcc against ctypes"""
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
    assert seen["vk_paths_info"] == (72,) and seen["vk_paths_step_info"] == (64,)
    n = 0
    for cname, T in STRUCTS.items():
        assert C.sizeof(T) == seen[cname][0]
        for f, _ in T._fields_:
            d = getattr(T, f)
            assert seen[f"{cname}.{f}"] == (d.offset, d.size), (cname, f)
            n += 1
    assert n == 6 + 9


def test_no_paths_function_takes_a_stream():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*paths\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args and "void *" not in args, fn
    assert seen == FUNCTIONS + ["vk_debug_compact_paths", "vk_debug_paths_last_ms"]


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    scene = C.c_void_p(0x1000)            # never read: each of these is refused first
    h = C.c_void_p(0x77)
    for args, word in (((None, 16, C.byref(h)), b"null argument"), ((scene, 16, None), b"null argument"),
                       ((scene, 0, C.byref(h)), b"capacity must be in 1..2^24"), ((scene, 2 ** 24 + 1, C.byref(h)), b"capacity must be in 1..2^24")):
        assert lib.vk_paths_create(*args) == ffi.VK_ERR_BAD_ARG, word
        assert word in lib.vk_last_error(), lib.vk_last_error()
    assert h.value == 0x77
    sp = ffi.ShadeParams(5, ffi.VK_INTEGRATOR_SCATTER, ffi.VK_BACKGROUND_SKY, ffi.F3(0, 0, 0), 0, 0)
    rays, states = np.zeros(4, RAY_DTYPE), np.zeros(4, PATH_STATE_DTYPE)
    assert lib.vk_paths_begin(None, C.byref(sp), rays.ctypes.data, states.ctypes.data, 4) == ffi.VK_ERR_BAD_ARG
    info, step = ffi.PathsInfo(), ffi.PathsStepInfo()
    info.capacity = step.traced = 99
    ids = np.full(4, 0x77, np.uint32)
    keep = np.ones(4, np.uint8)
    assert lib.vk_paths_step(None, 1, C.byref(step)) == ffi.VK_ERR_BAD_ARG and b"null path batch" in lib.vk_last_error()
    assert lib.vk_paths_read(None, ids.ctypes.data, None, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_paths_cull(None, keep.ctypes.data, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_paths_results(None, states.ctypes.data, ids.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_paths_get_info(None, C.byref(info)) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_paths_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert info.capacity == 99 and step.traced == 99 and (ids == 0x77).all() and not states.view(np.uint8).any()
    lib.vk_paths_destroy(None)            # nothing
    counts = (C.c_uint64 * 5)(*[7] * 5)
    assert lib.vk_debug_compact_paths(None, None, None, 0, 0, None, None, None, None, None, C.byref(counts)) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_compact_paths(scene, None, None, 0, 0, None, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_compact_paths(scene, None, None, 4, 4, None, None, None, None, None, C.byref(counts)) == ffi.VK_ERR_BAD_ARG
    assert list(counts) == [7] * 5
    ms = (C.c_double * 3)(7, 7, 7)
    assert lib.vk_debug_paths_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_paths_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7, 7]


def test_the_sizes_follow_the_kernel_constants():
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read()
    assert int(re.search(r"constexpr int PATHS_T = (\d+);", src).group(1)) == paths_ref.PATHS_T
    assert int(re.search(r"constexpr int PATHS_SCAN_T = (\d+);", src).group(1)) == paths_ref.PATHS_SCAN_T
    n_wg = -(-paths_ref.N_SCAN_TWO_PASSES // paths_ref.PATHS_T)
    assert n_wg > paths_ref.PATHS_SCAN_T and paths_ref.N_SCAN_TWO_PASSES <= 2 ** 20 and paths_ref.N_SCAN_TWO_PASSES % paths_ref.PATHS_T
    for n in (paths_ref.PATHS_T - 1, paths_ref.PATHS_T, paths_ref.PATHS_T + 1, 3 * paths_ref.PATHS_T + 5):
        assert n in paths_ref.SIZES


def test_the_kernels_are_new(built):
    """trace_paths_kernel<F> in trace_rays_kernel's two variants, the compaction's three kernels, the marking pass and the ids: no
    AGPRs, no dynamic stack; only the compaction's passes hold static LDS"""
    txt = open(build.kernel_resources_path()).read()
    seen = {}
    for blk in txt.split("Name: ")[1:]:
        name = blk.split("\n")[0]
        if "paths_" not in name:
            continue
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        assert name not in seen
        seen[name] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), occupancy=get("Occupancy [waves/SIMD]"),
                          lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk)
    trace = sorted(int(re.search(r"trace_paths_kernelILj(\d+)EE", k).group(1)) for k in seen if "trace_paths_kernel" in k)
    assert trace == [0, 0x17F], trace
    for k in ("paths_count_kernel", "paths_scan_kernel", "paths_move_kernel", "paths_cull_mark_kernel", "paths_iota_kernel"):
        assert sum(k in name for name in seen) == 1, k
    assert len(seen) == 7, sorted(seen)
    for name, r in seen.items():
        assert r["agprs"] == 0 and not r["dynamic_stack"] and r["occupancy"] >= 1, (name, r)
        assert (r["lds"] > 0) == any(k in name for k in ("paths_count", "paths_scan", "paths_move")), (name, r)
        assert r["lds"] <= 256, (name, r)
