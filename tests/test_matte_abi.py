"""ID mattes (vk_render_mattes, vk_matte_merge, vk_matte_mask: additive symbols of ABI 7) on the CPU: the four functions and the debug
hook declared, exported by both libraries, bound, declared in the Rust shim; vk_matte_params as gcc lays it out against the ctypes
mirror; no stream-taking function, no `void *`, and no name another family's pins would catch; the refusals that need no device, each
leaving its outputs untouched; vk_matte_merge and vk_matte_mask against tests/matte_ref.py on random tables; the kernels of vk_matte.hip
in a resource record of their own — exactly the new ones, without scratch, AGPRs, LDS or a dynamic stack."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import matte_ref
from descs import params
from vecchio_amd import build, ffi
from vecchio_amd.scene import matte_mask, matte_merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_matte_default_params", "vk_render_mattes", "vk_matte_merge", "vk_matte_mask"]
HOOKS = ["vk_debug_matte_samples"]
KERNELS = ["_ZN12_GLOBAL__N_112matte_kernelILj0EEEv9MatteArgs", "_ZN12_GLOBAL__N_112matte_kernelILj383EEEv9MatteArgs",
           "_ZN12_GLOBAL__N_120matte_samples_kernelILj0EEEv9MatteArgs", "_ZN12_GLOBAL__N_120matte_samples_kernelILj383EEEv9MatteArgs"]
FORBIDDEN = ("film", "paths", "regen", "adapt_", "roulette", "probe", "shade", "radiance", "irradiance", "splat")
SCRATCH_OPS_CEILING = 0     # as built: the table stays in registers across the walk
BG = ffi.VK_MATTE_BACKGROUND


def header(name="vecchio_amd.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_declared_exported_and_bound(built):
    hdr = header()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    for fn in FUNCTIONS:
        assert re.search(r"\bint " + fn + r"\s*\(", code(hdr)), fn
        assert fn in ffi.DEVICE_SYMBOLS, fn
    for fn in HOOKS:
        assert re.search(r"\bint " + fn + r"\s*\(", code(header("vecchio_amd_debug.h"))), fn
    for path in (ffi.device_lib_path(), build.build_device_debug()):
        lib = C.CDLL(path)
        for fn in FUNCTIONS + HOOKS:
            assert hasattr(lib, fn), (path, fn)
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7 == ffi.VK_ABI_VERSION
    common = [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_uint32]
    assert lib.vk_matte_default_params.argtypes == [C.POINTER(ffi.MatteParams)]
    assert lib.vk_render_mattes.argtypes == common + [C.POINTER(ffi.MatteParams)] + [C.c_void_p] * 3 + [C.POINTER(ffi.Stats)]
    assert lib.vk_matte_merge.argtypes == [C.c_uint32, C.c_uint64] + [C.c_void_p] * 6
    assert lib.vk_matte_mask.argtypes == [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    assert lib.vk_debug_matte_samples.argtypes == common + [C.c_uint32, C.c_void_p]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS + HOOKS)
    assert (ffi.VK_MATTE_OBJECT, ffi.VK_MATTE_MATERIAL, ffi.VK_MATTE_BACKGROUND, ffi.VK_MATTE_MAX_RANKS) == (0, 1, 0xFFFFFFFF, 8)
    assert re.search(r"enum \{ VK_MATTE_OBJECT = 0, VK_MATTE_MATERIAL = 1 \};", code(hdr))
    assert re.search(r"#define VK_MATTE_BACKGROUND 0xFFFFFFFFu\b", hdr) and re.search(r"#define VK_MATTE_MAX_RANKS 8u\b", hdr)
    assert matte_ref.BACKGROUND == BG and matte_ref.MAX_RANKS == 8


def test_default_params(built):
    lib = ffi.load_device_lib()
    mp = ffi.MatteParams(9, 9, 9, 9)
    assert lib.vk_matte_default_params(C.byref(mp)) == ffi.VK_OK
    assert (mp.kind, mp.ranks, mp.flags, mp._pad) == (ffi.VK_MATTE_OBJECT, 6, 0, 0)
    assert lib.vk_matte_default_params(None) == ffi.VK_ERR_BAD_ARG


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_matte_default_params": r"out: \*mut vk_matte_params\) -> c_int;",
        "vk_render_mattes": r"scene: \*mut vk_scene, cam: \*const vk_camera, params: \*const vk_render_params, first_sample: u32,\s+"
                            r"mp: \*const vk_matte_params, ids: \*mut u32, counts: \*mut u32, overflow: \*mut u32, "
                            r"stats_out: \*mut vk_stats\) -> c_int;",
        "vk_matte_merge": r"ranks: u32, n_pixels: u64, ids: \*mut u32, counts: \*mut u32, overflow: \*mut u32, ids_b: \*const u32,\s+"
                          r"counts_b: \*const u32, overflow_b: \*const u32\) -> c_int;",
        "vk_matte_mask": r"ranks: u32, n_pixels: u64, ids: \*const u32, counts: \*const u32, n_samples: u32, want: \*const u32, "
                         r"n_want: u32,\s+mask_out: \*mut f32\) -> c_int;",
    }
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    for n, v in (("VK_MATTE_OBJECT", "0"), ("VK_MATTE_MATERIAL", "1"), ("VK_MATTE_BACKGROUND", "0xFFFF_FFFF"), ("VK_MATTE_MAX_RANKS", "8")):
        assert re.search(rf"pub const {n}: u32 = {v};", rs), n
    m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct vk_matte_params\s*\{(.*?)\}", rs, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "pub kind: u32, pub ranks: u32, pub flags: u32, pub _pad: u32"
    import test_rust_shim_layout as R
    c, r = R.c_structs(), R.rust_structs()
    assert "vk_matte_params" in c and r.get("vk_matte_params") == c["vk_matte_params"]


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """vk_matte_params is 16 bytes, and every field's offset and size: the header through gcc against ctypes"""
    lines = ['printf("vk_matte_params %zu\\n", sizeof(vk_matte_params));']
    for f, _ in ffi.MatteParams._fields_:
        lines.append(f'printf("{f} %zu %zu\\n", offsetof(vk_matte_params, {f}), sizeof(((vk_matte_params *)0)->{f}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vecchio_amd.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    seen = {}
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            k, *v = ln.split()
            seen[k] = tuple(int(x) for x in v)
    assert seen["vk_matte_params"] == (16,) == (C.sizeof(ffi.MatteParams),)
    assert [f for f, _ in ffi.MatteParams._fields_] == ["kind", "ranks", "flags", "_pad"]
    for f, _ in ffi.MatteParams._fields_:
        d = getattr(ffi.MatteParams, f)
        assert seen[f] == (d.offset, d.size), f


def test_no_matte_function_takes_a_stream_and_no_other_pin_catches_one():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*matte\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args and "void *" not in args, fn
            assert not [w for w in FORBIDDEN if w in fn], fn
    assert seen == FUNCTIONS + HOOKS


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    cam, p = ffi.Camera(), params(16, 16, 4)
    cam.time0, cam.time1 = 0.0, 1.0
    ids, counts, over = (np.full(16 * 16 * 8, 7, np.uint32) for _ in range(3))
    I, N, O = (C.c_void_p(a.ctypes.data) for a in (ids, counts, over))
    ok = ffi.MatteParams(ffi.VK_MATTE_OBJECT, 6, 0, 0)
    call = lambda scene, mp, a, b, first=0, pp=p: lib.vk_render_mattes(scene, C.byref(cam), C.byref(pp), first,
                                                                       C.byref(mp) if mp is not None else None, a, b, O, None)
    for args, word in (((h, None, I, N), b"null matte parameters"), ((h, ok, None, N), b"null matte ids or counts"),
                       ((h, ok, I, None), b"null matte ids or counts"),
                       ((h, ffi.MatteParams(2, 6, 0, 0), I, N), b"unknown matte kind"),
                       ((h, ffi.MatteParams(0xFFFFFFFF, 6, 0, 0), I, N), b"unknown matte kind"),
                       ((h, ffi.MatteParams(0, 0, 0, 0), I, N), b"matte ranks must be in 1..8"),
                       ((h, ffi.MatteParams(1, 9, 0, 0), I, N), b"matte ranks must be in 1..8"),
                       ((h, ffi.MatteParams(0, 6, 1, 0), I, N), b"matte flags must be 0"),
                       ((None, ok, I, N), b"null argument")):
        assert call(*args) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), word
    assert lib.vk_render_mattes(h, None, C.byref(p), 0, C.byref(ok), I, N, O, None) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_render_mattes(h, C.byref(cam), None, 0, C.byref(ok), I, N, O, None) == ffi.VK_ERR_BAD_ARG
    # vk_render's checks, in its words, and the window's end
    for fields, word in ((dict(width=1), b"width and height must be >= 2"), (dict(samples_per_pixel=0), b"samples_per_pixel must be in 1..2^26"),
                         (dict(tile_world=2, tile_rank=2), b"tile_rank >= tile_world")):
        bad = params(16, 16, 4)
        for k, v in fields.items():
            setattr(bad, k, v)
        assert call(h, ok, I, N, pp=bad) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), fields
    assert call(h, ok, I, N, first=0xFFFFFFFF - 3) == ffi.VK_ERR_BAD_ARG and b"exceeds 2^32 - 1" in lib.vk_last_error()
    late = ffi.Camera()
    late.time0, late.time1 = 1.0, 1.0
    assert lib.vk_render_mattes(h, C.byref(late), C.byref(p), 0, C.byref(ok), I, N, O, None) == ffi.VK_ERR_BAD_ARG and b"time0 >= time1" in lib.vk_last_error()
    # the hook
    for args, word in (((h, C.byref(cam), C.byref(p), 0, 0, None), b"null matte ids"), ((h, C.byref(cam), C.byref(p), 0, 2, I), b"unknown matte kind"),
                       ((None, C.byref(cam), C.byref(p), 0, 0, I), b"null argument"),
                       ((h, C.byref(cam), C.byref(p), 0xFFFFFFFF, 0, I), b"exceeds 2^32 - 1")):
        assert lib.vk_debug_matte_samples(*args) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), word
    # merge and mask
    mask = np.full(4, 7, np.float32)
    M = C.c_void_p(mask.ctypes.data)
    want = np.array([7], np.uint32)
    W = C.c_void_p(want.ctypes.data)
    for args, word in (((0, 4, I, N, O, I, N, O), b"matte ranks must be in 1..8"), ((9, 4, I, N, O, I, N, O), b"matte ranks must be in 1..8"),
                       ((2, 4, None, N, O, I, N, O), b"null matte table"), ((2, 4, I, None, O, I, N, O), b"null matte table"),
                       ((2, 4, I, N, O, None, N, O), b"null matte table"), ((2, 4, I, N, O, I, None, O), b"null matte table"),
                       ((2, 4, I, N, O, I, N, None), b"both or neither"), ((2, 4, I, N, None, I, N, O), b"both or neither")):
        assert lib.vk_matte_merge(*args) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), args
    for args, word in (((0, 4, I, N, 4, W, 1, M), b"matte ranks must be in 1..8"), ((9, 4, I, N, 4, W, 1, M), b"matte ranks must be in 1..8"),
                       ((2, 4, I, N, 0, W, 1, M), b"n_samples must be >= 1"), ((2, 4, I, N, 4, None, 1, M), b"null matte id set"),
                       ((2, 4, None, N, 4, W, 1, M), b"null matte table"), ((2, 4, I, None, 4, W, 1, M), b"null matte table"),
                       ((2, 4, I, N, 4, W, 1, None), b"null matte table")):
        assert lib.vk_matte_mask(*args) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), args
    assert (ids == 7).all() and (counts == 7).all() and (over == 7).all() and (mask == 7).all()
    # nothing to do is not an error
    assert lib.vk_matte_merge(2, 0, None, None, None, None, None, None) == ffi.VK_OK
    assert lib.vk_matte_mask(2, 0, None, None, 4, None, 0, None) == ffi.VK_OK


# ---------------------------------------------------------------- merge and mask against the reference
POOL = np.array([0, 1, 2, 3, 0x20000005, 0x40000002, 0x60000001, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, BG], np.uint32)


def windows(seed, n_pixels, n_windows, spp, distinct):
    """per-sample ids (n_windows, n_pixels, spp): each pixel draws from its own `distinct` ids of POOL"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_windows, n_pixels, spp), np.uint32)
    for i in range(n_pixels):
        mine = rng.choice(POOL, size=int(rng.integers(1, distinct + 1)), replace=False)
        out[:, i, :] = rng.choice(mine, size=(n_windows, spp))
    return out


def equal(got, want, where=None):
    for g, w, what in zip(got, want, ("ids", "counts", "overflow")):
        np.testing.assert_array_equal(g if where is None else g[where], w if where is None else w[where], err_msg=what)


@pytest.mark.parametrize("ranks", [1, 2, 3, 8])
def test_merge_against_the_reference_and_its_contract(ranks, built):
    """three windows merged in all six orders: the library's merge is the reference's bit for bit, whatever the tables hold; wherever the
    one call over the union has overflow 0 every order gives that call's table, and the merged overflow is 0 exactly there"""
    n_pixels, spp = 160, 9
    ids3 = windows(40 + ranks, n_pixels, 3, spp, distinct=min(ranks + 2, len(POOL)))
    tables = [matte_ref.table(ids3[w], ranks) for w in range(3)]
    union = matte_ref.table(np.concatenate([ids3[0], ids3[1], ids3[2]], axis=-1), ranks)
    clean = union[2] == 0
    assert clean.any() and (~clean).any()                   # tables with and without overflow
    assert any((t[2] != 0).any() for t in tables) or ranks == 8
    for order in itertools.permutations(range(3)):
        a = tuple(x.copy() for x in tables[order[0]])
        want = tables[order[0]]
        for w in order[1:]:
            b = tuple(x.copy() for x in tables[w])
            matte_merge(*a, *b)
            equal(b, tables[w])                              # b is read only
            want = matte_ref.merge(want, tables[w])
            equal(a, want)
        equal(a, union, clean)
        np.testing.assert_array_equal(a[2] == 0, clean)
        assert (a[1].sum(-1) + a[2] == 3 * spp).all()
    # without the overflow arrays: the same slots
    a = tuple(x.copy() for x in tables[0])
    matte_merge(a[0], a[1], None, tables[1][0].copy(), tables[1][1].copy(), None)
    w = matte_ref.merge(tables[0], tables[1])
    np.testing.assert_array_equal(a[0], w[0])
    np.testing.assert_array_equal(a[1], w[1])
    np.testing.assert_array_equal(a[2], tables[0][2])


@pytest.mark.parametrize("ranks", [1, 2, 3, 8])
def test_mask_against_the_reference(ranks, built):
    n_pixels, spp = 200, 13
    ids = windows(70 + ranks, n_pixels, 1, spp, distinct=6)[0]
    t = matte_ref.table(ids, ranks)
    for want in ([], [BG], [0], [1, 2, 3], list(POOL), [0x7FFFFFFF, 0x80000000, 12345]):
        got = matte_mask(t[0], t[1], spp, want)
        ref = matte_ref.mask(t[0], t[1], spp, want)
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=str(want))
    # every id wanted: what the table kept of the pixel
    np.testing.assert_array_equal(matte_mask(t[0], t[1], spp, list(POOL)), ((spp - t[2]).astype(np.float32) / np.float32(spp)))
    # closed form, by hand: two slots of three and one of seven samples, a free slot
    ids1 = np.array([[5, 9, 2, 0]], np.uint32)
    counts1 = np.array([[7, 3, 3, 0]], np.uint32)
    assert matte_mask(ids1, counts1, 16, [9, 2])[0] == np.float32(6) / np.float32(16)
    assert matte_mask(ids1, counts1, 16, [0])[0] == 0.0 and matte_mask(ids1, counts1, 13, [5, 0])[0] == np.float32(7) / np.float32(13)


def test_reference_by_hand():
    """tests/matte_ref.py itself on a case worked out by hand from the header's text"""
    seq = np.array([[4, 9, 4, BG, 7, 9, 9, 7, 3]], np.uint32)
    ids, counts, over = matte_ref.table(seq, 3)
    # slots taken in order 4, 9, BG; then 7, 7 and 3 overflow; 9 x3, 4 x2, BG x1
    assert ids.tolist() == [[9, 4, BG]] and counts.tolist() == [[3, 2, 1]] and over.tolist() == [3]
    ids, counts, over = matte_ref.table(seq, 8)
    assert ids.tolist() == [[9, 4, 7, 3, BG, 0, 0, 0]] and counts.tolist() == [[3, 2, 2, 1, 1, 0, 0, 0]] and over.tolist() == [0]
    a = (np.array([[9, 4]], np.uint32), np.array([[3, 2]], np.uint32), np.array([1], np.uint32))
    b = (np.array([[7, 4]], np.uint32), np.array([[5, 1]], np.uint32), np.array([2], np.uint32))
    ids, counts, over = matte_ref.merge(a, b)
    assert ids.tolist() == [[4, 9]] and counts.tolist() == [[3, 3]] and over.tolist() == [8]


# ---------------------------------------------------------------- the kernels' resource record
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
    """kernel_resources_matte.txt lists exactly the kernels of vk_matte.hip, each once: no dynamic stack, no AGPRs, no LDS, the scratch
    instructions as built as a ceiling (none: the table is eight register pairs across the walk); the other three records hold none"""
    mine = resources(build.kernel_resources_matte_path())
    assert sorted(mine) == sorted(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert not [w for w in FORBIDDEN if w in name.lower()], name
        assert r["agprs"] == 0 and r["lds"] == 0 and not r["dynamic_stack"], (name, r)
        assert 0 <= r["scratch_ops"] <= SCRATCH_OPS_CEILING, (name, r)
    for path in (build.kernel_resources_path(), build.kernel_resources_adapt_path(), build.kernel_resources_splat_path()):
        assert not [n for n in resources(path) if "matte" in n.lower()] and "matte" not in open(path).read().lower()
