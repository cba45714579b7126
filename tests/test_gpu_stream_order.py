"""Every entry point that takes a `hip_stream`, on a non-blocking stream of the caller's own, behind a delay, with no host wait
(tests/stream_order.py says how a mis-ordered enqueue becomes a wrong value).  TABLE names, per entry point of the two headers, the tests
that drive it this way; tests/test_stream_order_table.py holds the table to the headers.  The expected values are those of the same call
on the NULL stream between two device synchronisations, which the other GPU tests hold to numpy and the oracle bit for bit.

Each check prints one line `STREAM_ORDER {...}` (pytest -s): the delay asked for and measured and the call's own synchronous time, in ms.
They are for the record (profiles/stream_order/report.jsonl), nothing is asserted of them."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import denoise_ref
import rays_ref
import stream_order as so
import temporal_ref
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

TABLE = {
    "vk_render_device": ("test_render_device", "test_render_device_on_the_dual_launch", "test_a_pipeline_on_one_stream"),
    "vk_to_color_device": ("test_to_color_device", "test_a_pipeline_on_one_stream"),
    "vk_pack_tiles_device": ("test_pack_and_unpack_tiles_device",),
    "vk_unpack_tiles_device": ("test_pack_and_unpack_tiles_device",),
    "vk_progress_step_device": ("test_progress_windows_back_to_back",),
    "vk_progress_stderr_device": ("test_progress_windows_back_to_back",),
    "vk_render_aov_device": ("test_first_hit_buffers", "test_a_pipeline_on_one_stream"),
    "vk_render_guides_device": ("test_first_hit_buffers",),
    "vk_trace_rays_device": ("test_trace_rays_device", "test_a_pipeline_on_one_stream"),
    "vk_trace_occluded_device": ("test_trace_occluded_device", "test_a_misordered_call_is_seen"),
    "vk_debug_trace_occluded_device": ("test_debug_trace_occluded_device",),
    "vk_denoise_device": ("test_denoise_device", "test_a_misordered_call_is_seen", "test_a_pipeline_on_one_stream"),
    "vk_temporal_accumulate_device": ("test_temporal_frames_back_to_back", "test_a_pipeline_on_one_stream"),
}

PREFILL = {np.float32: (so.CANARY_F32, 3.0), np.uint8: (so.CANARY_BYTE, 0x55)}     # dtype -> (what a framebuffer holds, its poison)
SEED = 0xC0FFEE12345


# ---------------------------------------------------------------- shared pieces
@pytest.fixture(scope="module")
def S(device):
    import torch
    return torch.cuda.Stream()


_scenes = {}


def scene(host_scenes, name, devices=None, lib=None):
    key = (name, tuple(devices) if devices else None, lib is not None)
    if key not in _scenes:
        hs, cam = host_scenes(name)
        _scenes[key] = DeviceScene(hs.desc, devices=devices, lib=lib)
    hs, cam = host_scenes(name)
    return hs, cam, _scenes[key]


def other_camera(cam):
    """another valid camera: what the struct handed to a call is overwritten with when the call has returned"""
    c = so.clone(cam)
    for k in range(3):
        c.origin[k] += 1.0 + k
        c.lower_left_corner[k] -= 0.5
    return c


def other_params(p):
    q = so.clone(p)
    q.seed += 12345
    q.samples_per_pixel += 3
    q.max_depth = 2
    q.tile_rank, q.tile_world = 0, 1
    return q


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def empty(shape, dtype=np.float32):
    import torch
    return torch.zeros(shape, dtype={np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}[dtype], device="cuda:0")


def ok(lib, status):
    assert status == ffi.VK_OK, lib.vk_last_error().decode()


class Case:
    """One check: `inputs` with their `true` values and `poison`, `outputs`, and call(ctx).  begin() / end(): what a pass needs fresh (a
    handle with history).  head_witness: per output what a call enqueued AHEAD of its inputs leaves in the copy, where the poison run
    cannot tell (a buffer that is prefilled and then written: its prefill) — None = the poison run's outputs."""
    inputs = true = poison = outputs = ()
    names = None
    head_witness = None
    delay_ms = so.DELAY_MS

    def begin(self):
        pass

    def end(self):
        pass

    def call(self, ctx):
        raise NotImplementedError

    def after(self):
        pass


def run_case(case, S, what):
    """reference run, poison run (condition (b)), ordered run (condition (a) inside); returns (got, ref)"""
    case.begin()
    try:
        ref, sync_ms = so.reference_call(case.inputs, case.true, case.call, case.outputs)
    finally:
        case.end()
    case.begin()
    try:
        wrong, _ = so.reference_call(case.inputs, case.poison, case.call, case.outputs)
    finally:
        case.end()
    witness = wrong if case.head_witness is None else case.head_witness
    assert not so.same(ref, witness), f"{what}: VACUOUS — a call that ran ahead of its inputs would give the reference's values"
    for w in (witness, wrong):
        for r, x in zip(ref, w):
            assert r.shape == x.shape
    case.begin()
    try:
        got = so.ordered_call(S, case.inputs, case.poison, case.call, case.outputs, true=case.true, delay_ms=case.delay_ms)
        print("\nSTREAM_ORDER " + json.dumps({"row": what, "delay_asked_ms": case.delay_ms, "delay_measured_ms": round(so.measured_delay_ms(case.delay_ms), 3),
                                              "delay_by": so._cal["kind"], "call_sync_ms": round(sync_ms, 3)}))
        assert so.same(got, ref), f"{what}: the ordered run differs from the reference run — " + so.describe_difference(got, ref, case.names) + \
            ("; it EQUALS the poison run" if so.same(got, wrong) else "")
        case.after()
    finally:
        case.end()
    return got, ref


def tile_mask(width, height, rank, world, top_down=False):
    """(height, width) bool: the pixels of the 8x8 tiles t with t % world == rank, in the image's row order"""
    tiles_x = (width + 7) // 8
    y = np.arange(height)[::-1] if top_down else np.arange(height)
    return ((y[:, None] // 8) * tiles_x + np.arange(width)[None, :] // 8) % world == rank


# ---------------------------------------------------------------- vk_render_device
class RenderCase(Case):
    def __init__(self, ds, cam, p):
        dt = np.uint8 if p.output_format == ffi.VK_OUTPUT_RGB8 else np.float32
        self.ds, self.cam, self.p = ds, cam, p
        self.fb = empty((p.height, p.width, 3), dt)
        prefill, poison = PREFILL[dt]
        self.inputs, self.true, self.poison, self.outputs, self.names = [self.fb], [prefill], [poison], [self.fb], ["framebuffer"]
        self.head_witness = [np.full((p.height, p.width, 3), prefill, dt)]

    def call(self, ctx):
        cam, p = so.clone(self.cam), so.clone(self.p)
        self.ds.render_device(cam, p, self.fb.data_ptr(), ctx.ptr)
        ctx.mark()
        so.overwrite(cam, other_camera(self.cam))
        so.overwrite(p, other_params(self.p))


RENDER_SCENES = ("cornell_box", "random_spheres_iow", "final_scene")


@pytest.mark.parametrize("layout", ["one_device", "two_parts", "rank_1_of_3"])
@pytest.mark.parametrize("fmt", [ffi.VK_OUTPUT_F32, ffi.VK_OUTPUT_RGB8], ids=["f32", "rgb8"])
@pytest.mark.parametrize("name", RENDER_SCENES)
def test_render_device(name, fmt, layout, device, host_scenes, S):
    hs, cam, ds = scene(host_scenes, name, devices=[0, 0] if layout == "two_parts" else None)
    rank, world = (1, 3) if layout == "rank_1_of_3" else (0, 1)
    p = hs.params(64, 8, 50, seed=5, height=48, tile_rank=rank, tile_world=world, output_format=fmt)
    case = RenderCase(ds, cam, p)
    got, ref = run_case(case, S, f"vk_render_device {name} {'rgb8' if fmt else 'f32'} {layout}")
    # the reference itself: the blocking call's image, and nothing outside the partition
    host, _ = ds.render(cam, p, out=np.full((48, 64, 3), PREFILL[ref[0].dtype.type][0], ref[0].dtype))
    assert so.same(ref, [host])
    mine = tile_mask(64, 48, rank, world, top_down=fmt == ffi.VK_OUTPUT_RGB8)
    assert (got[0][~mine] == PREFILL[ref[0].dtype.type][0]).all() and (got[0][mine] != PREFILL[ref[0].dtype.type][0]).any()
    if name == "random_spheres_iow" and layout == "one_device":
        # the grid form: the frame had the second launch, the fallback launch behind it and the asynchronous copy of its plan
        assert ds.info().tree == ffi.VK_TREE_REBUILT_GRID
        roles = {r.role for r in ffi.last_launches(ds._lib, ds._h)}
        assert {ffi.VK_LAUNCH_REDO, ffi.VK_LAUNCH_FALLBACK} <= roles, roles


def test_render_device_on_the_dual_launch(device, host_scenes, S, monkeypatch):
    """the recipe of test_gpu_adaptive.py::test_the_scenes_later_behaviour_is_untouched: the second stream's fork from and join into S"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-cus * 112 // 24)
    width, height = 320, 8 * -(-tiles // 40)
    hs, cam = host_scenes("random_spheres_iow")
    monkeypatch.setenv("VK_CHUNK_CAP", "1")          # (read at scene creation: a unit per tile and sample)
    ds = DeviceScene(hs.desc)
    monkeypatch.delenv("VK_CHUNK_CAP")
    try:
        case = RenderCase(ds, cam, hs.params(width, 24, 50, height=height))
        run_case(case, S, "vk_render_device dual launch")
        roles = {r.role for r in ffi.last_launches(ds._lib, ds._h)}             # (of the ordered run, the scene's last frame)
        assert {ffi.VK_LAUNCH_DUAL_1024, ffi.VK_LAUNCH_DUAL_768} <= roles, roles
    finally:
        ds.close()


# ---------------------------------------------------------------- vk_progress_step_device, vk_progress_stderr_device
class ProgressCase(Case):
    WINDOWS, SPP = 4, 4

    def __init__(self, ds, cam, p, adaptive):
        self.ds, self.cam, self.p, self.adaptive = ds, cam, p, adaptive
        shape = (p.height, p.width, 3)
        self.fb = empty(shape)
        self.snaps = [empty(shape) for _ in range(self.WINDOWS)]
        self.se = empty(shape)
        self.inputs, self.true, self.poison = [self.fb], [PREFILL[np.float32][0]], [PREFILL[np.float32][1]]
        self.outputs = self.snaps + [self.se]
        self.names = [f"window {i}" for i in range(self.WINDOWS)] + ["stderr"]
        full = np.full(shape, so.CANARY_F32, f32)
        self.head_witness = [full] * (self.WINDOWS + 1)

    def begin(self):
        self.pr = self.ds.progress(self.cam, self.p, stderr=True, adaptive=self.adaptive)

    def end(self):
        self.pr.close()

    def call(self, ctx):
        for i in range(self.WINDOWS):
            self.pr.step_device(self.SPP, self.fb.data_ptr(), ctx.ptr)
            ctx.copy_out(self.snaps[i], self.fb)
        ctx.mark()            # (vk_progress_stderr_device waits on the host for the last step, as documented: (a) is the steps')
        self.pr.stderr_device(self.se.data_ptr(), ctx.ptr)


@pytest.mark.parametrize("adaptive", [None, dict(abs_tol=0.05, rel_tol=0.0, min_samples=0, min_steps=2)], ids=["plain", "adaptive"])
def test_progress_windows_back_to_back(adaptive, device, host_scenes, S):
    hs, cam, ds = scene(host_scenes, "random_spheres_iow")
    p = hs.params(64, ProgressCase.WINDOWS * ProgressCase.SPP, 50, seed=5, height=48)
    case = ProgressCase(ds, cam, p, adaptive)
    got, ref = run_case(case, S, f"vk_progress_step_device x4 + vk_progress_stderr_device {'adaptive' if adaptive else 'plain'}")
    # the reference itself: the blocking handle's images
    with ds.progress(cam, p, stderr=True, adaptive=adaptive) as pr:
        host = [pr.step(ProgressCase.SPP)[0].copy() for _ in range(ProgressCase.WINDOWS)] + [pr.stderr()]
        if adaptive:
            inf = pr.tile_samples()[1]
            assert 0 < inf.tiles_active < inf.tiles_total, "the adaptive case froze no tile, or all of them"
    assert so.same(ref, host)


# ---------------------------------------------------------------- vk_render_aov_device, vk_render_guides_device
class FirstHitCase(Case):
    def __init__(self, ds, cam, p, guides, channels):
        self.ds, self.cam, self.p, self.guides = ds, cam, p, guides
        n = p.width * p.height
        sizes = [3 * n, 3 * n, n, n] + ([n] if guides else [])
        self.slab = empty((sum(sizes) + 64,))              # the channels side by side: an absent one's room, and the tail, stay as prefilled
        at = np.concatenate([[0], np.cumsum(sizes)])
        self.ptrs = [self.slab.data_ptr() + 4 * int(at[i]) if i in channels else 0 for i in range(len(sizes))]
        self.untouched = np.ones(sum(sizes) + 64, bool)
        for i in channels:
            self.untouched[at[i]:at[i + 1]] = False
        self.inputs, self.true, self.poison, self.outputs, self.names = [self.slab], [PREFILL[np.float32][0]], [PREFILL[np.float32][1]], [self.slab], ["slab"]
        self.head_witness = [np.full(self.slab.shape, so.CANARY_F32, f32)]
        self.gp = ds.guide_params() if guides else None

    def call(self, ctx):
        cam, p = so.clone(self.cam), so.clone(self.p)
        if self.guides:
            gp = so.clone(self.gp)
            self.ds.render_guides_device(cam, p, 0, gp, *self.ptrs, stream=ctx.ptr)
            ctx.mark()
            so.overwrite(gp, self.ds.guide_params(max_bounces=1, fuzz_max=0.5))
        else:
            self.ds.render_aov_device(cam, p, 0, *self.ptrs, stream=ctx.ptr)
            ctx.mark()
        so.overwrite(cam, other_camera(self.cam))
        so.overwrite(p, other_params(self.p))


@pytest.mark.parametrize("channels", ["every_buffer", "albedo_only"])
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
@pytest.mark.parametrize("entry", ["vk_render_aov_device", "vk_render_guides_device"])
def test_first_hit_buffers(entry, name, channels, device, host_scenes, S):
    hs, cam, ds = scene(host_scenes, name)
    guides = entry == "vk_render_guides_device"
    p = hs.params(24, 4, 50, seed=7, height=16)             # samples 0..3
    chans = (0,) if channels == "albedo_only" else tuple(range(5 if guides else 4))
    case = FirstHitCase(ds, cam, p, guides, chans)
    got, ref = run_case(case, S, f"{entry} {name} {channels}")
    assert (got[0][case.untouched] == so.CANARY_F32).all(), "memory next to the wanted buffers was written"
    names = DeviceScene.GUIDE_CHANNELS if guides else DeviceScene.AOV_CHANNELS
    host = (ds.render_guides(cam, p, 0, want=[names[i] for i in chans]) if guides else ds.render_aov(cam, p, 0, want=[names[i] for i in chans]))[0]
    n = 24 * 16
    assert np.array_equal(so.bits(ref[0][:3 * n]), so.bits(host["albedo"].reshape(-1)))


# ---------------------------------------------------------------- vk_trace_rays_device, vk_trace_occluded_device and its debug twin
OCC_K = int(re.search(r"constexpr uint32_t OCC_K = (\d+)u", open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read()).group(1))


@pytest.fixture(scope="module")
def final_scene_rays(oracle, host_scenes):
    hs, cam = host_scenes("final_scene")
    rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
    return rays


def rays_away(n):
    """poison rays: valid, and nothing of any scene lies that way"""
    from vecchio_amd.scene import make_rays
    return make_rays(np.tile(f32([0, 1e6, 0]), (n, 1)), np.tile(f32([0, 1, 0]), (n, 1)))


def as_floats(rays):
    return np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()


class TraceCase(Case):
    """entry(lib, handle, tp, d_rays, n, d_out, stream) -> status"""

    def __init__(self, ds, rays, entry, out_shape, out_dtype, pad=0):
        self.ds, self.entry, self.n = ds, entry, len(rays)
        self.d_rays = empty((self.n, 8))
        self.buf = empty(out_shape, out_dtype)
        self.out_ptr = self.buf.data_ptr() + pad
        self.inputs, self.true, self.poison = [self.d_rays], [dev(as_floats(rays))], [dev(as_floats(rays_away(self.n)))]
        self.outputs, self.names = [self.buf], ["results"]
        self.tp = ffi.TraceParams(SEED, 7, 0, 0)

    def call(self, ctx):
        tp = so.clone(self.tp)
        ok(self.ds._lib, self.entry(self.ds._lib, self.ds._h, tp, self.d_rays.data_ptr(), self.n, self.out_ptr, ctx.ptr))
        ctx.mark()
        so.overwrite(tp, ffi.TraceParams(SEED + 1, 1000, 0, 0))


def _trace_rays(lib, h, tp, d_rays, n, d_out, stream):
    return lib.vk_trace_rays_device(h, C.byref(tp), C.c_void_p(d_rays), n, C.c_void_p(d_out), C.c_void_p(stream or 0), None)


def _trace_occluded(lib, h, tp, d_rays, n, d_out, stream):
    return lib.vk_trace_occluded_device(h, C.byref(tp), C.c_void_p(d_rays), n, C.c_void_p(d_out), C.c_void_p(stream or 0), None)


def occluded_case(ds, rays, entry=_trace_occluded):
    n = 64 * OCC_K + 1
    return TraceCase(ds, np.resize(rays, n), entry, (n + 129,), np.uint8, pad=1)      # (an odd address, canaries on both sides)


def test_trace_rays_device(device, host_scenes, final_scene_rays, S):
    hs, cam, ds = scene(host_scenes, "final_scene")
    case = TraceCase(ds, final_scene_rays, _trace_rays, (len(final_scene_rays), 16), np.int32)
    got, ref = run_case(case, S, "vk_trace_rays_device final_scene")
    host = ds.trace_rays(final_scene_rays, SEED, 7)
    rays_ref.assert_bit_identical(ref[0].view(np.uint32).reshape(-1).view(host.dtype), host, "the reference run against vk_trace_rays")
    assert host["medium"].any() and 0 < host["hit"].sum() < len(host)


def test_trace_occluded_device(device, host_scenes, final_scene_rays, S):
    hs, cam, ds = scene(host_scenes, "final_scene")
    case = occluded_case(ds, final_scene_rays)
    got, ref = run_case(case, S, f"vk_trace_occluded_device final_scene {case.n} rays")
    host = ds.trace_occluded(np.resize(final_scene_rays, case.n), SEED, 7)
    assert np.array_equal(ref[0][1:1 + case.n], host) and (got[0][0] == so.CANARY_BYTE) and (got[0][1 + case.n:] == so.CANARY_BYTE).all()


@pytest.mark.parametrize("refill,k,t", [(0, 0, 0), (1, 1, 64)], ids=["one_ray_per_lane", "refill_k1_t64"])
def test_debug_trace_occluded_device(refill, k, t, device, host_scenes, final_scene_rays, S):
    hs, cam, dd = scene(host_scenes, "final_scene", lib=ffi.load_debug_lib())
    entry = lambda lib, h, tp, d_rays, n, d_out, stream: lib.vk_debug_trace_occluded_device(
        h, C.byref(tp), C.c_void_p(d_rays), n, C.c_void_p(d_out), C.c_void_p(stream or 0), refill, k, t)
    case = occluded_case(dd, final_scene_rays, entry)
    got, ref = run_case(case, S, f"vk_debug_trace_occluded_device final_scene refill {refill} k {k} t {t}")
    _, _, ds = scene(host_scenes, "final_scene")
    assert np.array_equal(ref[0][1:1 + case.n], ds.trace_occluded(np.resize(final_scene_rays, case.n), SEED, 7))


# ---------------------------------------------------------------- vk_denoise_device
DN_KEYS = ("color", "stderr3", "albedo", "normal", "depth")


class DenoiseCase(Case):
    def __init__(self, ds, g, form, levels=4):
        h, w = g["color"].shape[:2]
        self.ds, self.form = ds, form
        self.dp = ds.denoise_params(w, h, levels=levels)
        self.bufs = {k: empty(g[k].shape) for k in DN_KEYS}
        self.out = empty((h, w, 3))
        self.inputs, self.true, self.poison = [self.bufs[k] for k in DN_KEYS], [dev(g[k]) for k in DN_KEYS], [0.0] * 5
        self.outputs, self.names = [self.out], ["out"]

    def begin(self):
        ok(self.ds._lib, self.ds._lib.vk_debug_denoise_form(self.ds._h, self.form))

    def end(self):
        self.ds._lib.vk_debug_denoise_form(self.ds._h, ffi.VK_DENOISE_FORM_AUTO)

    def call(self, ctx):
        dp, b = so.clone(self.dp), self.bufs
        self.ds.denoise_device(dp, b["color"].data_ptr(), self.out.data_ptr(), b["stderr3"].data_ptr(), b["albedo"].data_ptr(),
                               b["normal"].data_ptr(), b["depth"].data_ptr(), stream=ctx.ptr)
        ctx.mark()
        so.overwrite(dp, self.ds.denoise_params(self.dp.width, self.dp.height, levels=1, sigma_l=0.5))


@pytest.mark.parametrize("form", [ffi.VK_DENOISE_FORM_PLAIN, ffi.VK_DENOISE_FORM_STAGED], ids=["plain", "staged"])
def test_denoise_device(form, device, host_scenes, S):
    hs, cam, ds = scene(host_scenes, "cornell_box")
    g = denoise_ref.synthetic(37, 29)
    got, ref = run_case(DenoiseCase(ds, g, form), S, f"vk_denoise_device 37x29 4 levels {'staged' if form == ffi.VK_DENOISE_FORM_STAGED else 'plain'}")
    host, _ = ds.denoise(g["color"], g["stderr3"], g["albedo"], g["normal"], g["depth"], params=ds.denoise_params(37, 29, levels=4))
    assert so.same(ref, [host])


# ---------------------------------------------------------------- vk_temporal_accumulate_device
TA_IN = ("color", "stderr3", "albedo", "normal", "depth")


class TemporalCase(Case):
    def __init__(self, ds, seq, w, h):
        self.ds, self.w, self.h = ds, w, h
        self.cams = [temporal_ref.to_ffi(cam) for cam, _ in seq]
        self.frames = [{k: empty(g[k].shape) for k in TA_IN} for _, g in seq]
        self.outs = [(empty((h, w, 3)), empty((h, w, 3)), empty((h, w))) for _ in seq]
        self.inputs = [f[k] for f in self.frames for k in TA_IN]
        self.true = [dev(g[k]) for _, g in seq for k in TA_IN]
        self.poison = [0.0] * len(self.inputs)
        self.outputs = [o for frame in self.outs for o in frame]
        self.names = [f"frame {i} {what}" for i in range(len(seq)) for what in ("colour", "stderr", "history")]
        self.history = []

    def begin(self):
        self.t = self.ds.temporal(self.w, self.h)

    def end(self):
        self.history.append(self.t.info().pixels_with_history)      # (waits for the last frame: after the pass)
        self.t.close()

    def call(self, ctx):
        for cam0, f, (oc, ose, on) in zip(self.cams, self.frames, self.outs):
            cam = so.clone(cam0)
            self.t.accumulate_device(cam, f["color"].data_ptr(), f["normal"].data_ptr(), f["depth"].data_ptr(), oc.data_ptr(),
                                     d_stderr=f["stderr3"].data_ptr(), d_albedo=f["albedo"].data_ptr(), d_out_stderr=ose.data_ptr(),
                                     d_out_history=on.data_ptr(), stream=ctx.ptr)
            so.overwrite(cam, other_camera(cam0))
            ctx.barrier()
        ctx.mark()


def test_temporal_frames_back_to_back(device, host_scenes, S):
    hs, cam, ds = scene(host_scenes, "cornell_box")
    w, h = 37, 29
    seq = temporal_ref.synthetic(w, h, frames=3)
    case = TemporalCase(ds, seq, w, h)
    got, ref = run_case(case, S, "vk_temporal_accumulate_device x3 37x29")
    true_history, poison_history, ordered_history = case.history
    assert ordered_history == true_history and true_history > 0
    with ds.temporal(w, h) as t:                                     # the reference itself: the blocking handle's frames
        host = []
        for cam_i, g in seq:
            host += list(t.accumulate(temporal_ref.to_ffi(cam_i), g["color"], g["normal"], g["depth"], stderr=g["stderr3"], albedo=g["albedo"],
                                      want_history=True)[:3])
        assert t.info().pixels_with_history == true_history
    assert so.same(ref, host)


# ---------------------------------------------------------------- vk_to_color_device, vk_pack_tiles_device, vk_unpack_tiles_device
W0, H0 = 37, 29


def an_image(seed=3):
    return np.random.default_rng(seed).uniform(0.0, 1.2, (H0, W0, 3)).astype(f32)


class ToColorCase(Case):
    def __init__(self, ds):
        self.ds = ds
        self.rgb, self.rgb8 = empty((H0, W0, 3)), empty((H0, W0, 3), np.uint8)
        self.inputs, self.true, self.poison, self.outputs, self.names = [self.rgb], [dev(an_image())], [0.0], [self.rgb8], ["rgb8"]

    def call(self, ctx):
        self.ds.to_color_device(self.rgb.data_ptr(), W0, H0, self.rgb8.data_ptr(), stream=ctx.ptr)


def test_to_color_device(device, host_scenes, S):
    hs, cam, ds = scene(host_scenes, "cornell_box")
    got, ref = run_case(ToColorCase(ds), S, "vk_to_color_device 37x29")
    want = (np.clip(np.sqrt(an_image().astype(np.float64)), 0.0, 0.999) * 256.0).astype(np.int64)[::-1]      # vec3.rs:54-61, top row first
    assert np.abs(ref[0].astype(np.int64) - want).max() <= 1          # (to the byte next door: the f32 square root's last bit is not this test's)


class PackCase(Case):
    RANK, WORLD = 1, 3

    def __init__(self, ds, fmt):
        self.ds, self.fmt = ds, fmt
        self.fb = empty((H0, W0, 3))
        self.slab = empty((ds._lib.vk_tile_slab_bytes(W0, H0, fmt, self.RANK, self.WORLD) + 64,), np.uint8)
        self.inputs, self.true, self.poison, self.outputs, self.names = [self.fb], [dev(an_image())], [0.0], [self.slab], ["slab"]

    def call(self, ctx):
        self.ds.pack_tiles_device(self.fb.data_ptr(), W0, H0, self.fmt, self.RANK, self.WORLD, self.slab.data_ptr(), stream=ctx.ptr)


class UnpackCase(Case):
    def __init__(self, ds, fmt, slab_bytes):
        self.ds, self.fmt = ds, fmt
        dt = np.uint8 if fmt == ffi.VK_OUTPUT_RGB8 else np.float32
        self.slab, self.img = empty(slab_bytes.shape, np.uint8), empty((H0, W0, 3), dt)
        prefill, poison = PREFILL[dt]
        self.inputs, self.true, self.poison = [self.slab, self.img], [dev(slab_bytes), prefill], [0, poison]
        self.outputs, self.names = [self.img], ["image"]

    def call(self, ctx):
        self.ds.unpack_tiles_device(self.slab.data_ptr(), W0, H0, self.fmt, PackCase.RANK, PackCase.WORLD, self.img.data_ptr(), stream=ctx.ptr)


@pytest.mark.parametrize("fmt", [ffi.VK_OUTPUT_F32, ffi.VK_OUTPUT_RGB8], ids=["f32", "rgb8"])
def test_pack_and_unpack_tiles_device(fmt, device, host_scenes, S):
    hs, cam, ds = scene(host_scenes, "cornell_box")
    what = "rgb8" if fmt else "f32"
    got, slab = run_case(PackCase(ds, fmt), S, f"vk_pack_tiles_device 37x29 {what} rank 1 of 3")
    assert (slab[0][-64:] == so.CANARY_BYTE).all()
    got, img = run_case(UnpackCase(ds, fmt, slab[0]), S, f"vk_unpack_tiles_device 37x29 {what} rank 1 of 3")
    # the round trip itself: this rank's tiles of the image (through to_color for RGB8), nothing else touched
    rgb8 = fmt == ffi.VK_OUTPUT_RGB8
    mine = tile_mask(W0, H0, PackCase.RANK, PackCase.WORLD, top_down=rgb8)
    assert (img[0][~mine] == PREFILL[img[0].dtype.type][0]).all()
    if not rgb8:
        assert np.array_equal(so.bits(img[0][mine]), so.bits(an_image()[mine]))


# ---------------------------------------------------------------- the use case: a frame's whole chain on one stream
class PipelineCase(Case):
    """render A -> first-hit buffers -> temporal -> denoise -> to_color -> ray query -> render B, every stage's output copied out behind
    it; nothing but S orders them"""
    W, H = 64, 48

    def __init__(self, hs, ds, cam_a, cam_b, rays):
        w, h = self.W, self.H
        self.ds, self.cam_a, self.cam_b = ds, cam_a, cam_b
        self.pa, self.pb = hs.params(w, 8, 50, seed=5, height=h), hs.params(w, 8, 50, seed=6, height=h)
        self.fb, self.albedo, self.normal, self.depth = empty((h, w, 3)), empty((h, w, 3)), empty((h, w, 3)), empty((h, w))
        self.acc, self.dn, self.rgb8 = empty((h, w, 3)), empty((h, w, 3)), empty((h, w, 3), np.uint8)
        self.d_rays, self.hits = empty((len(rays), 8)), empty((len(rays), 16), np.int32)
        self.dp, self.tp = ds.denoise_params(w, h, levels=3), ffi.TraceParams(SEED, 0, 0, 0)
        stages = [("frame A", self.fb), ("albedo", self.albedo), ("normal", self.normal), ("depth", self.depth), ("accumulated", self.acc),
                  ("denoised", self.dn), ("rgb8", self.rgb8), ("hits", self.hits), ("frame B", self.fb)]
        self.names = [n for n, _ in stages]
        self.snaps = [empty(tuple(b.shape), {"torch.uint8": np.uint8, "torch.int32": np.int32}.get(str(b.dtype), np.float32)) for _, b in stages]
        self.inputs, self.true, self.poison = [self.d_rays, self.fb], [dev(as_floats(rays)), so.CANARY_F32], [dev(as_floats(rays_away(len(rays)))), 3.0]
        self.outputs = self.snaps

    def begin(self):
        self.t = self.ds.temporal(self.W, self.H)
        for b in (self.albedo, self.normal, self.depth, self.acc, self.dn, self.rgb8, self.hits):
            so.fill(b, so.canary_of(b))

    def end(self):
        self.t.close()

    def call(self, ctx):
        ds, st = self.ds, ctx.ptr
        cam, p = so.clone(self.cam_a), so.clone(self.pa)
        ds.render_device(cam, p, self.fb.data_ptr(), st)
        ctx.barrier()
        ds.render_aov_device(cam, p, 0, self.albedo.data_ptr(), self.normal.data_ptr(), self.depth.data_ptr(), stream=st)
        ctx.barrier()
        self.t.accumulate_device(cam, self.fb.data_ptr(), self.normal.data_ptr(), self.depth.data_ptr(), self.acc.data_ptr(),
                                 d_albedo=self.albedo.data_ptr(), stream=st)
        so.overwrite(cam, other_camera(self.cam_a))
        so.overwrite(p, other_params(self.pa))
        ctx.copy_out(self.snaps[0], self.fb)
        dp = so.clone(self.dp)
        ds.denoise_device(dp, self.acc.data_ptr(), self.dn.data_ptr(), d_albedo=self.albedo.data_ptr(), d_normal=self.normal.data_ptr(),
                          d_depth=self.depth.data_ptr(), stream=st)
        so.overwrite(dp, ds.denoise_params(self.W, self.H, levels=1))
        ctx.barrier()
        ds.to_color_device(self.dn.data_ptr(), self.W, self.H, self.rgb8.data_ptr(), stream=st)
        for i, b in ((1, self.albedo), (2, self.normal), (3, self.depth), (4, self.acc), (5, self.dn), (6, self.rgb8)):
            ctx.copy_out(self.snaps[i], b)
        tp = so.clone(self.tp)
        ok(ds._lib, _trace_rays(ds._lib, ds._h, tp, self.d_rays.data_ptr(), self.d_rays.shape[0], self.hits.data_ptr(), st))
        so.overwrite(tp, ffi.TraceParams(SEED + 1, 5, 0, 0))
        ctx.copy_out(self.snaps[7], self.hits)
        cam, p = so.clone(self.cam_b), so.clone(self.pb)
        ds.render_device(cam, p, self.fb.data_ptr(), st)
        ctx.mark()
        so.overwrite(cam, other_camera(self.cam_b))
        so.overwrite(p, other_params(self.pb))
        ctx.copy_out(self.snaps[8], self.fb)


def test_a_pipeline_on_one_stream(device, oracle, host_scenes, S):
    hs, cam_a, ds = scene(host_scenes, "cornell_box")
    cam_b = other_camera(cam_a)
    rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam_a, hs.params(24, 1, 50, seed=7, height=16)))
    case = PipelineCase(hs, ds, cam_a, cam_b, rays)
    first, _ = ds.render(cam_a, case.pa)
    got, ref = run_case(case, S, "pipeline: render, aov, temporal, denoise, to_color, trace_rays, render")
    assert so.same([ref[0]], [first]) and not so.same([ref[8]], [first])
    again, _ = ds.render(cam_a, case.pa)                             # the scene's scratch came through
    assert so.same([again], [first])


# ---------------------------------------------------------------- the harness sees a mis-ordered enqueue
@pytest.mark.parametrize("entry", ["vk_trace_occluded_device", "vk_denoise_device"])
def test_a_misordered_call_is_seen(entry, device, host_scenes, final_scene_rays, S):
    """the same sequence with the library call on a second stream while its inputs arrive on S: valid buffers, valid work, wrong order —
    the copy holds the poison run's values or the canary, never the reference's"""
    if entry == "vk_denoise_device":
        hs, cam, ds = scene(host_scenes, "cornell_box")
        case = DenoiseCase(ds, denoise_ref.synthetic(37, 29), ffi.VK_DENOISE_FORM_AUTO)
    else:
        hs, cam, ds = scene(host_scenes, "final_scene")
        case = occluded_case(ds, final_scene_rays)
    S2 = so.concurrent_stream(S)
    assert S2 is not None, "no second stream runs alongside S on this device: the self-test cannot be made"
    case.begin()
    try:
        ref, _ = so.reference_call(case.inputs, case.true, case.call, case.outputs)
        wrong, _ = so.reference_call(case.inputs, case.poison, case.call, case.outputs)
        assert not so.same(ref, wrong)
        got = so.ordered_call(S, case.inputs, case.poison, case.call, case.outputs, true=case.true, library_stream=S2)
    finally:
        case.end()
    canary = np.full_like(got[0], so.canary_of_numpy(got[0]))
    assert not so.same(got, ref), f"{entry}: a call enqueued on another stream went unnoticed"
    assert so.same(got, wrong) or so.same(got, [canary]), so.describe_difference(got, wrong, case.names)
