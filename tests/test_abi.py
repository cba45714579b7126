"""The C-ABI library: loads, exports every symbol include/vecchio_amd.h declares, agrees with the
ctypes mirror on struct layout, and FAILS LOUDLY without a GPU (there is no CPU path).
No compute calls here — those are the -m gpu tests."""
import ctypes as C
import os
import re
import subprocess

from vecchio_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vecchio_amd.h")
HEADERS = sorted(os.path.join(ROOT, "include", f) for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))


def declared_functions():
    """every function declared in include/*.h (the boundary and the debug header)"""
    names = set()
    for h in HEADERS:
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names |= set(re.findall(r"\b(vk_[a-z_0-9]+)\s*\(", src))
    return sorted(names)


def test_exports_every_declared_symbol(built):
    names = declared_functions()
    assert {"vk_scene_create", "vk_render", "vk_render_device", "vk_scene_destroy", "vk_last_error", "vk_abi_version",
            "vk_device_count", "vk_to_color_device", "vk_scene_create_multi", "vk_debug_render_samples"} <= set(names)
    lib = C.CDLL(ffi.device_lib_path())
    # the diagnostic entry points of vecchio_amd_debug.h that need instrumented kernel builds, and the live-object counter, live in
    # libvecchio_amd_debug.so (the same sources with -DVK_DEBUG_LIB), which exports everything; the product library exports everything
    # else and NOT those
    debug_only = {"vk_debug_phase_stats", "vk_debug_math", "vk_debug_live_objects"}
    missing = [n for n in names if not hasattr(lib, n) and n not in debug_only]
    assert not missing, f"declared in include/*.h but not exported by the product library: {missing}"
    assert not [n for n in debug_only if hasattr(lib, n)]
    from vecchio_amd import build
    dbg = C.CDLL(build.build_device_debug())
    assert not [n for n in names if not hasattr(dbg, n)]
    assert set(ffi.DEVICE_SYMBOLS) <= set(names)


def test_abi_version_and_error_string(built):
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == ffi.VK_ABI_VERSION
    assert isinstance(lib.vk_last_error(), bytes)


def test_struct_layout_matches_header(built, tmp_path):
    names = {"vk_bvh_node": ffi.BvhNode, "vk_sphere": ffi.Sphere, "vk_moving_sphere": ffi.MovingSphere, "vk_rect": ffi.Rect,
             "vk_list": ffi.List, "vk_medium": ffi.Medium, "vk_translate": ffi.Translate, "vk_rotate": ffi.Rotate,
             "vk_material": ffi.Material, "vk_texture": ffi.Texture, "vk_image": ffi.Image, "vk_perlin": ffi.Perlin,
             "vk_scene_desc": ffi.SceneDesc, "vk_camera": ffi.Camera, "vk_render_params": ffi.RenderParams,
             "vk_stats": ffi.Stats, "vk_scene_info": ffi.SceneInfo, "vk_part_info": ffi.PartInfo}
    src = tmp_path / "sz.c"
    body = "\n".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
    src.write_text(f'#include <stdio.h>\n#include "{HEADER}"\nint main(){{ {body} return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)]).decode().split()
    sizes = dict(zip(out[0::2], map(int, out[1::2])))
    for n, T in names.items():
        assert C.sizeof(T) == sizes[n], f"{n}: ctypes {C.sizeof(T)} vs C {sizes[n]}"
    assert sizes["vk_bvh_node"] == 32      # the canonical 32-byte node record


def test_launch_log_layout_matches_debug_header(built, tmp_path):
    """vk_debug_launch (include/vecchio_amd_debug.h) and its VK_LAUNCH_* roles against the ctypes mirror, field by field"""
    hdr = os.path.join(ROOT, "include", "vecchio_amd_debug.h")
    fields = [f[0] for f in ffi.DebugLaunch._fields_]
    roles = ["VK_LAUNCH_MAIN", "VK_LAUNCH_DUAL_1024", "VK_LAUNCH_DUAL_768", "VK_LAUNCH_PROBE", "VK_LAUNCH_REDO", "VK_LAUNCH_FALLBACK"]
    body = 'printf("sizeof %zu\\n", sizeof(vk_debug_launch));' + "".join(
        f'printf("{f} %zu\\n", offsetof(vk_debug_launch, {f}));' for f in fields) + "".join(f'printf("{r} %d\\n", (int){r});' for r in roles)
    src = tmp_path / "launch.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{hdr}"\nint main(){{ {body} return 0; }}\n')
    exe = tmp_path / "launch"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)]).decode().split()
    got = dict(zip(out[0::2], map(int, out[1::2])))
    assert got["sizeof"] == C.sizeof(ffi.DebugLaunch)
    for f in fields:
        assert got[f] == getattr(ffi.DebugLaunch, f).offset, f
    for r in roles:
        assert got[r] == getattr(ffi, r), r
    lib = ffi.load_device_lib()
    assert lib.vk_debug_last_launches.argtypes[1] is C.POINTER(ffi.DebugLaunch)
    n = C.c_uint32(7)
    assert lib.vk_debug_last_launches(None, None, 0, C.byref(n)) == ffi.VK_ERR_BAD_ARG       # (no scene: refused, nothing written)
    assert n.value == 7


def test_rccl_gather_backend_resolves_without_being_linked(built):
    """VK_SCENE_RCCL_GATHER (ABI 6): the in-library gather of a multi-device scene as grouped ncclSend / ncclRecv (north_star: "RCCL over
    xGMI only for the final framebuffer gather").  librccl.so is loaded on request — the product library must not depend on it — and
    every entry point the code path calls must resolve (the compile-and-link check of a path no one-GPU box can run)."""
    import subprocess
    lib = ffi.load_device_lib()
    assert lib.vk_gather_backends() & 1
    assert lib.vk_gather_backends() & 2, "librccl.so (or one of ncclCommInitAll/ncclSend/ncclRecv/...) does not resolve on this image"
    needed = subprocess.run(["ldd", ffi.device_lib_path()], capture_output=True, text=True).stdout
    assert "rccl" not in needed and "nccl" not in needed, needed


def test_no_cpu_fallback(built):
    """Without a usable gfx950 device scene creation must fail with an error, never render."""
    lib = ffi.load_device_lib()
    if lib.vk_device_count() > 0:
        return   # on the GPU box the -m gpu tests cover the real path
    from vecchio_amd import HostScene
    hs = HostScene("cornell_box", 1)
    h = C.c_void_p()
    st = lib.vk_scene_create(hs.desc, 0, C.byref(h))
    assert st in (ffi.VK_ERR_NO_DEVICE, ffi.VK_ERR_HIP) and not h.value
    assert len(lib.vk_last_error()) > 0


def test_product_does_not_reference_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may touch oracle/ (or tests/emu)."""
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "vecchio_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".h", ".hip", ".rs")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                if re.search(r'#include\s*"[^"\n]*(oracle|emu)|import\s+(oracle|emu)|liboracle|libemu|dlopen\([^)\n]*(oracle|emu)', txt):
                    if f != "build.py":       # build.py only COMPILES the checker (allowed: build() builds it)
                        bad.append(os.path.join(base, f))
    assert not bad, bad
