"""Adaptive sampling at the C boundary, checked without a GPU: vk_progress_set_adaptive, vk_progress_tile_samples and the test hook
vk_debug_progress_moments are declared and exported (additive symbols: VK_ABI_VERSION stays 7), the two records agree with their ctypes
and Rust twins, and the entry points reject null handles.  What they compute is tests/test_gpu_adaptive.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vecchio_amd.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "vecchio_amd_debug.h")
SHIM = os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")

FUNCTIONS = ["vk_progress_set_adaptive", "vk_progress_tile_samples"]


def declared(path, fn):
    return re.search(rf"\b{fn}\s*\(", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))


def test_declared_and_exported(built):
    for fn in FUNCTIONS:
        assert declared(HEADER, fn), f"{fn} not declared in vecchio_amd.h"
    assert declared(DEBUG_HEADER, "vk_debug_progress_moments")
    assert set(FUNCTIONS) <= set(ffi.DEVICE_SYMBOLS)
    from vecchio_amd import build
    for path in (ffi.device_lib_path(), build.build_device_debug()):
        lib = C.CDLL(path)
        missing = [fn for fn in FUNCTIONS + ["vk_debug_progress_moments"] if not hasattr(lib, fn)]
        assert not missing, f"{os.path.basename(path)} does not export {missing}"


def test_abi_version_stays_7(built):
    assert re.search(r"#define VK_ABI_VERSION 7\b", open(HEADER).read())
    assert ffi.VK_ABI_VERSION == 7 and ffi.load_device_lib().vk_abi_version() == 7


def test_struct_layouts(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\n'
                   'int main(){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(vk_adaptive_params), '
                   'offsetof(vk_adaptive_params, abs_tol), offsetof(vk_adaptive_params, rel_tol), offsetof(vk_adaptive_params, min_samples), '
                   'offsetof(vk_adaptive_params, min_steps), sizeof(vk_adaptive_info), offsetof(vk_adaptive_info, tiles_total), '
                   'offsetof(vk_adaptive_info, tiles_active), offsetof(vk_adaptive_info, samples_rendered)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).decode().split()))
    A, I = ffi.AdaptiveParams, ffi.AdaptiveInfo
    want = [C.sizeof(A), A.abs_tol.offset, A.rel_tol.offset, A.min_samples.offset, A.min_steps.offset,
            C.sizeof(I), I.tiles_total.offset, I.tiles_active.offset, I.samples_rendered.offset]
    assert got == want == [16, 0, 4, 8, 12, 16, 0, 4, 8]


def test_rust_twins():
    import test_rust_shim_layout as R
    c, r = R.c_structs(), R.rust_structs()
    for name in ("vk_adaptive_params", "vk_adaptive_info"):
        assert name in c and r.get(name) == c[name], name
    shim = open(SHIM).read()
    for fn in FUNCTIONS:
        assert re.search(rf"pub fn {fn}\(", shim), fn


def test_null_handles_rejected(built):
    lib = ffi.load_device_lib()
    ap = ffi.AdaptiveParams(1e-3, 0.0, 0, 2)
    assert lib.vk_progress_set_adaptive(None, C.byref(ap)) == ffi.VK_ERR_BAD_ARG
    out = np.zeros(16, np.uint32)
    info = ffi.AdaptiveInfo()
    assert lib.vk_progress_tile_samples(None, out.ctypes.data_as(C.c_void_p), C.byref(info)) == ffi.VK_ERR_BAD_ARG
    run = np.zeros(48, np.int64)
    assert lib.vk_debug_progress_moments(None, run.ctypes.data_as(C.c_void_p), None) == ffi.VK_ERR_BAD_ARG
    assert len(lib.vk_last_error()) > 0
