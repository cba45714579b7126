"""Python handles over the two product libraries.

HostScene  = a scene built by the C++ mirror of scene.rs (libvecchio_host.so) and flattened
             into a vk_scene_desc (what the Rust shim's flatten() would hand over).
DeviceScene = that description uploaded through the C ABI (vk_scene_create) to one MI355X;
             render() is one call of the drop-in for main.rs:181-198.
Progress   = one frame of a DeviceScene accumulated over successive sample windows (vk_progress_*).
Temporal   = the frames of a moving camera reprojected and blended into a history (vk_temporal_*).
"""
import ctypes as C

import numpy as np

from . import ffi


class HostScene:
    def __init__(self, name, seed=1):
        self._lib = ffi.load_host_lib()
        self._h = self._lib.vkh_scene_build(name.encode(), seed)
        if not self._h:
            raise RuntimeError(self._lib.vkh_last_error().decode())
        self.name = name
        self.desc = self._lib.vkh_scene_desc(self._h)  # POINTER(SceneDesc), owned by the handle
        ar, integ, bg = C.c_float(), C.c_uint32(), C.c_uint32()
        col = ffi.F3()
        self._lib.vkh_scene_defaults(self._h, C.byref(ar), C.byref(integ), C.byref(bg), col)
        self.aspect_ratio = ar.value
        self.integrator = integ.value
        self.background = bg.value
        self.background_color = tuple(col)

    def next_camera(self):
        cam = ffi.Camera()
        if not self._lib.vkh_scene_next_camera(self._h, C.byref(cam)):
            return None
        return cam

    def params(self, width, spp, max_depth, seed=2, height=None, tile_rank=0, tile_world=1, output_format=ffi.VK_OUTPUT_F32):
        """vk_render_params with the scene's integrator/background; height = width/aspect (main.rs:172)."""
        p = ffi.RenderParams()
        p.width = width
        p.height = height if height is not None else int(np.float32(width) / np.float32(self.aspect_ratio))
        p.samples_per_pixel = spp
        p.max_depth = max_depth
        p.seed = seed
        p.integrator = self.integrator
        p.background = self.background
        p.background_color = ffi.F3(*self.background_color)
        p.tile_rank = tile_rank
        p.tile_world = tile_world
        p.output_format = output_format
        return p

    def close(self):
        if self._h:
            self._lib.vkh_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# numpy twins of vk_ray and vk_hit (DeviceScene.trace_rays)
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmax", "<f4"), ("direction", "<f4", 3), ("time", "<f4")])
HIT_DTYPE = np.dtype([("p", "<f4", 3), ("t", "<f4"), ("normal", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("hit", "<u4"), ("front", "<u4"),
                      ("material", "<u4"), ("object", "<u4"), ("medium", "<u4"), ("_pad", "<u4", 2)])
KEY_DTYPE = np.dtype([("seed", "<u8"), ("pixel", "<u4"), ("sample", "<u4"), ("ctr", "<u4"), ("_pad", "<u4")])   # vk_debug_stream_key
assert KEY_DTYPE.itemsize == C.sizeof(ffi.DebugStreamKey) == 24
assert RAY_DTYPE.itemsize == C.sizeof(ffi.Ray) == 32 and HIT_DTYPE.itemsize == C.sizeof(ffi.Hit) == 64
# numpy twins of vk_path_state and vk_shaded (DeviceScene.shade_hits)
PATH_STATE_DTYPE = np.dtype([("thr", "<f4", 3), ("depth", "<u4"), ("acc", "<f4", 3), ("counter", "<u4"), ("seed", "<u8"), ("pixel", "<u4"),
                             ("sample", "<u4")])
SHADED_DTYPE = np.dtype([("next", RAY_DTYPE), ("state", PATH_STATE_DTYPE), ("status", "<u4"), ("lobe", "<u4"), ("_pad", "<u4", 2)])
assert PATH_STATE_DTYPE.itemsize == C.sizeof(ffi.PathState) == 48 and SHADED_DTYPE.itemsize == C.sizeof(ffi.Shaded) == 96


def make_rays(origin, direction, time=0.0, tmax=np.inf):
    """A RAY_DTYPE array from origins and directions (n, 3) and per-ray or scalar times and tmax."""
    origin = np.asarray(origin, np.float32).reshape(-1, 3)
    rays = np.zeros(origin.shape[0], RAY_DTYPE)
    rays["origin"] = origin
    rays["direction"] = np.asarray(direction, np.float32).reshape(-1, 3)
    rays["time"] = time
    rays["tmax"] = tmax
    return rays


def make_path_states(n, seed=0, first_index=0, sample=0):
    """Fresh path states for DeviceScene.shade_hits(): a PATH_STATE_DTYPE array — thr 1, depth 1, acc 0, counter 0 — on the streams
    vk_trace_radiance gives sample `sample` of rays first_index .. first_index + n - 1 of a batch: seed + 0x9E3779B97F4A7C15 * index in
    wrapping u64, pixel 0."""
    st = np.zeros(n, PATH_STATE_DTYPE)
    st["thr"] = 1.0
    st["depth"] = 1
    mask = 0xFFFFFFFFFFFFFFFF
    st["seed"] = np.array([((seed & mask) + 0x9E3779B97F4A7C15 * (first_index + i)) & mask for i in range(n)], np.uint64)
    st["sample"] = sample
    return st


def wavefront_loop(trace, shade, rays, states, trace_seed=0, first_index=0):
    """The loop of vk_shade_hits' contract around two callables: hits = trace(rays, seed, first_index) (a HIT_DTYPE array) and
    out = shade(rays, hits, states) (a SHADED_DTYPE array), repeated on out["next"], out["state"] for the items whose status is
    VK_SHADE_SCATTERED.  trace_seed, first_index: of the media's streams; bounce b traces its live items, compacted, from index
    first_index + b * n, so that no two segments share a stream.
    Returns (states, bounces): the final PATH_STATE_DTYPE array in the order of `rays`, and per bounce a dict with the live items'
    indices, their rays, hits, states and results (the callables' arrays)."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1).copy()
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1).copy()
    assert rays.shape == states.shape
    n = rays.shape[0]
    live = np.arange(n)
    final = states.copy()
    bounces = []
    while live.size:
        hits = trace(rays, trace_seed, first_index + len(bounces) * n)
        out = shade(rays, hits, states)
        bounces.append({"index": live, "rays": rays, "hits": hits, "states": states, "out": out})
        final[live] = out["state"]
        go = out["status"] == ffi.VK_SHADE_SCATTERED
        live, rays, states = live[go], np.ascontiguousarray(out["next"][go]), np.ascontiguousarray(out["state"][go])
    return final, bounces


def make_points(p, normal, time=0.0, tmax=np.inf):
    """Points for DeviceScene.trace_irradiance(): a RAY_DTYPE array whose origin is the position and whose direction is the surface
    normal (of any non-zero length), from positions and normals (n, 3) and per-point or scalar times and tmax."""
    return make_rays(p, normal, time, tmax)


def points_from_hits(hits, time=0.0):
    """Points for DeviceScene.trace_irradiance() from trace_rays()' HIT_DTYPE records: the hit point with the normal that faces the ray
    that found it (vk_hit.normal is face-oriented already).  Misses and hits inside a medium (whose normal is arbitrary) are skipped;
    returns (points, index) with index[k] the record points[k] came from.  time: scalar, or one value per record."""
    hits = np.asarray(hits).reshape(-1)
    index = np.flatnonzero((hits["hit"] == 1) & (hits["medium"] == 0))
    time = np.broadcast_to(np.asarray(time, np.float32), hits.shape)[index]
    return make_points(hits["p"][index], hits["normal"][index], time), index


def make_probes(p, time=0.0, tmax=np.inf):
    """Probes for DeviceScene.trace_probes(): a RAY_DTYPE array whose origin is the position (the direction is not read), from positions
    (n, 3) and per-probe or scalar times and tmax."""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    return make_rays(p, np.zeros_like(p), time, tmax)


def probe_eval(sh, normal, mode=1, lib=None):
    """vk_probe_eval for one probe: sh (9, 3) as trace_probes() returns it, normal of any non-zero length.  mode 0: the band-limited
    radiance arriving along the normal; mode 1: irradiance / pi for it (what trace_irradiance() estimates).  A (3,) float32 array."""
    lib = lib or ffi.load_device_lib()
    sh = np.ascontiguousarray(sh, np.float32).reshape(27)
    n = (C.c_float * 3)(*[float(v) for v in np.asarray(normal, np.float32).reshape(3)])
    rgb = (C.c_float * 3)()
    check(lib, lib.vk_probe_eval(sh.ctypes.data_as(C.POINTER(C.c_float)), n, mode, rgb))
    return np.array(list(rgb), np.float32)


def check(lib, status):
    if status != ffi.VK_OK:
        raise RuntimeError(f"vecchio_amd status {status}: {lib.vk_last_error().decode()}")


def _matte_table(ids, counts, overflow):
    """a matte table's arrays as vk_matte_* take them: uint32, contiguous, (..., ranks) with one overflow per pixel or none"""
    for a in (ids, counts) + (() if overflow is None else (overflow,)):
        assert a.dtype == np.uint32 and a.flags.c_contiguous
    ranks = ids.shape[-1]
    assert counts.shape == ids.shape and (overflow is None or overflow.shape == ids.shape[:-1])
    return ranks, ids.size // ranks


def matte_merge(ids, counts, overflow, ids_b, counts_b, overflow_b, lib=None):
    """vk_matte_merge: folds table b into table a IN PLACE (host code, no device).  The tables are what DeviceScene.render_mattes()
    returns, for windows of one frame: (..., ranks) uint32 ids and counts, and per-pixel overflow arrays — both given or both None.
    Merged in any order, a frame's windows equal the one call over their union wherever that call's overflow is 0."""
    lib = lib or ffi.load_device_lib()
    ranks, n = _matte_table(ids, counts, overflow)
    assert _matte_table(ids_b, counts_b, overflow_b) == (ranks, n)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    check(lib, lib.vk_matte_merge(ranks, n, ptr(ids), ptr(counts), ptr(overflow), ptr(ids_b), ptr(counts_b), ptr(overflow_b)))
    return ids, counts, overflow


def matte_mask(ids, counts, n_samples, want, lib=None):
    """vk_matte_mask: the share of a pixel's n_samples samples whose id is one of `want` (a set, because one box is six face ids), as a
    float32 array of the table's pixel shape."""
    lib = lib or ffi.load_device_lib()
    ranks, n = _matte_table(ids, counts, None)
    want = np.ascontiguousarray(want, np.uint32).reshape(-1)
    out = np.zeros(ids.shape[:-1], np.float32)
    check(lib, lib.vk_matte_mask(ranks, n, C.c_void_p(ids.ctypes.data), C.c_void_p(counts.ctypes.data), n_samples,
                                 C.c_void_p(want.ctypes.data) if len(want) else None, len(want), C.c_void_p(out.ctypes.data)))
    return out


class DeviceScene:
    def __init__(self, desc, device=0, devices=None, lib=None):
        """device: one MI355X (vk_scene_create).  devices=[...]: one handle over several (vk_scene_create_multi):
        render() then deals the tiles over them and gathers on devices[0] inside the library.
        lib: another build of the library (ffi.load_debug_lib(): the handle belongs to the library that made it)."""
        self._lib = lib or ffi.load_device_lib()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            check(self._lib, self._lib.vk_scene_create_multi(desc, arr, len(devices), C.byref(h)))
            device = devices[0]
        else:
            check(self._lib, self._lib.vk_scene_create(desc, device, C.byref(h)))
        self._h = h
        self.device = device

    def info(self):
        inf = ffi.SceneInfo()
        check(self._lib, self._lib.vk_scene_get_info(self._h, C.byref(inf)))
        return inf

    def render(self, cam, params, out=None):
        """Blocking render into a host numpy array (height, width, 3): float32 with y = 0 the bottom row, or
        (params.output_format == VK_OUTPUT_RGB8) uint8 with row 0 the top row."""
        dt = np.uint8 if params.output_format == ffi.VK_OUTPUT_RGB8 else np.float32
        if out is None:
            out = np.zeros((params.height, params.width, 3), dtype=dt)
        assert out.dtype == dt
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_render(self._h, C.byref(cam), C.byref(params), out.ctypes.data_as(C.c_void_p), C.byref(stats)))
        return out, stats

    AOV_CHANNELS = ("albedo", "normal", "depth", "coverage")

    def render_aov(self, cam, params, first_sample=0, want=AOV_CHANNELS, out=None):
        """First-hit buffers of samples [first_sample, first_sample + params.samples_per_pixel) (vk_render_aov): a dict with the wanted
        channels as float32 arrays, y = 0 the bottom row — albedo and normal (height, width, 3), depth and coverage (height, width) —
        and the stats.  out: a dict of arrays to write into (pixels outside this call's tile partition keep their values)."""
        want = tuple(want)
        unknown = set(want) - set(self.AOV_CHANNELS)
        if unknown:
            raise ValueError(f"unknown AOV channel(s) {sorted(unknown)}; choose from {self.AOV_CHANNELS}")
        bufs = dict(out or {})
        for ch in want:
            if ch not in bufs:
                shape = (params.height, params.width, 3) if ch in ("albedo", "normal") else (params.height, params.width)
                bufs[ch] = np.zeros(shape, dtype=np.float32)
            assert bufs[ch].dtype == np.float32 and bufs[ch].flags.c_contiguous
        ptrs = [C.c_void_p(bufs[ch].ctypes.data) if ch in want else None for ch in self.AOV_CHANNELS]
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_render_aov(self._h, C.byref(cam), C.byref(params), first_sample, *ptrs, C.byref(stats)))
        return {ch: bufs[ch] for ch in want}, stats

    def render_aov_device(self, cam, params, first_sample, d_albedo=0, d_normal=0, d_depth=0, d_coverage=0, stream=None):
        """Enqueue the first-hit buffers into device memory (vk_render_aov_device, no host sync); a 0 pointer = not wanted."""
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_render_aov_device(self._h, C.byref(cam), C.byref(params), first_sample, C.c_void_p(d_albedo or None),
                                                        C.c_void_p(d_normal or None), C.c_void_p(d_depth or None),
                                                        C.c_void_p(d_coverage or None), C.c_void_p(stream or 0), C.byref(stats)))
        return stats

    def trace_rays(self, rays, seed=0, first_index=0, out=None, stream=None, return_stats=False):
        """Closest hits of caller-supplied rays (vk_trace_rays): rays is a RAY_DTYPE array (make_rays()) or anything of 32 bytes per
        ray that views as one; returns a HIT_DTYPE array, hits[i] answering rays[i].  Device tensors (objects with data_ptr(): a
        (n, 8) float32 tensor of rays on this scene's device) go through vk_trace_rays_device on `stream` without a host wait and
        return an (n, 16) int32 tensor — view it as HIT_DTYPE after copying it to the host — or write into `out`."""
        return self._trace_walk("vk_trace_rays", rays, seed, first_index, out, stream, return_stats, HIT_DTYPE, "int32", 16,
                                "device hits must be a contiguous int32 tensor of 16 words per ray")

    def trace_occluded(self, rays, seed=0, first_index=0, out=None, stream=None, return_stats=False):
        """Is anything between tmin and tmax of each caller-supplied ray (vk_trace_occluded): a uint8 array, occluded[i] == the `hit`
        field trace_rays() returns for rays[i].  rays as for trace_rays(): a RAY_DTYPE array, or a device tensor ((n, 8) float32 on this
        scene's device), which goes through vk_trace_occluded_device on `stream` without a host wait and returns an (n,) uint8 tensor
        (or writes into `out`).  Visibility of the segment from a to b: origin a, direction b - a, tmax 1."""
        return self._trace_walk("vk_trace_occluded", rays, seed, first_index, out, stream, return_stats, np.uint8, "uint8", 1,
                                "device occlusion bytes must be a contiguous uint8 tensor of one byte per ray")

    def _trace_walk(self, call, rays, seed, first_index, out, stream, return_stats, host_dtype, dev_dtype, dev_words, dev_out_error):
        """trace_rays() / trace_occluded(): the host call `call` for a numpy batch (one host_dtype record per ray), `call`_device on
        `stream` for a device tensor (dev_words elements of torch dtype dev_dtype per ray)"""
        tp = ffi.TraceParams(seed & 0xFFFFFFFFFFFFFFFF, first_index, 0, 0)
        stats = ffi.Stats()
        if hasattr(rays, "data_ptr"):
            import torch
            if rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 8 != 0:
                raise ValueError("device rays must be a contiguous float32 tensor of 8 floats per ray")
            n = rays.numel() // 8
            dev_dtype = getattr(torch, dev_dtype)
            if out is None:
                out = torch.empty((n, dev_words) if dev_words > 1 else (n,), dtype=dev_dtype, device=rays.device)
            if out.dtype != dev_dtype or not out.is_contiguous() or out.numel() != n * dev_words:
                raise ValueError(dev_out_error)
            check(self._lib, getattr(self._lib, call + "_device")(self._h, C.byref(tp), C.c_void_p(rays.data_ptr() if n else None), n,
                                                                  C.c_void_p(out.data_ptr() if n else None), C.c_void_p(stream or 0),
                                                                  C.byref(stats)))
            return (out, stats) if return_stats else out
        rays = self._host_rays(rays)
        if out is None:
            out = np.zeros(rays.shape[0], host_dtype)
        assert out.dtype == host_dtype and out.flags.c_contiguous and out.shape == rays.shape
        self._host_batch(call, tp, stats, rays, out)
        return (out, stats) if return_stats else out

    def _host_batch(self, call, params, stats, rays, *arrays):
        """the host-pointer call `call` for the n rays of `rays` with the further per-ray arrays (None = a null pointer); with n == 0
        every pointer is null"""
        n = rays.shape[0]
        ptrs = [C.c_void_p(a.ctypes.data if a is not None and n else None) for a in (rays,) + arrays]
        check(self._lib, getattr(self._lib, call)(self._h, C.byref(params), ptrs[0], n, *ptrs[1:], C.byref(stats)))

    @staticmethod
    def _host_rays(rays):
        rays = np.ascontiguousarray(rays)
        if rays.dtype != RAY_DTYPE:
            if rays.nbytes % 32 != 0 or rays.dtype.itemsize not in (4, 32):
                raise ValueError("rays must be a RAY_DTYPE array (or float32 data of 8 floats per ray)")
            rays = rays.reshape(-1).view(RAY_DTYPE)
        return rays.reshape(-1)

    @staticmethod
    def radiance_params(seed=0, first_index=0, samples_per_ray=1, first_sample=0, max_depth=50, integrator=ffi.VK_INTEGRATOR_PDF,
                        background=ffi.VK_BACKGROUND_SOLID, background_color=(0.0, 0.0, 0.0)):
        """A vk_radiance_params (ffi.RadianceParams)."""
        return ffi.RadianceParams(seed & 0xFFFFFFFFFFFFFFFF, first_index, samples_per_ray, first_sample, max_depth, integrator, background,
                                  ffi.F3(*background_color), 0, 0)

    def trace_radiance(self, rays, seed=0, first_index=0, samples_per_ray=1, first_sample=0, max_depth=50,
                       integrator=ffi.VK_INTEGRATOR_PDF, background=ffi.VK_BACKGROUND_SOLID, background_color=(0.0, 0.0, 0.0), out=None,
                       return_stats=False):
        """Path-traced colour arriving along caller-supplied rays (vk_trace_radiance): an (n, 3) float32 array, out[i] the mean of
        samples first_sample .. first_sample + samples_per_ray - 1 of rays[i], each ray_color(rays[i]) on its own stream.  rays as for
        trace_rays(): a RAY_DTYPE array (host memory; the call has no device-pointer variant yet)."""
        rp = self.radiance_params(seed, first_index, samples_per_ray, first_sample, max_depth, integrator, background, background_color)
        stats = ffi.Stats()
        rays = self._host_rays(rays)
        n = rays.shape[0]
        if out is None:
            out = np.zeros((n, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (n, 3)
        self._host_batch("vk_trace_radiance", rp, stats, rays, out)
        return (out, stats) if return_stats else out

    @staticmethod
    def shade_params(max_depth=50, integrator=ffi.VK_INTEGRATOR_PDF, background=ffi.VK_BACKGROUND_SOLID, background_color=(0.0, 0.0, 0.0)):
        """A vk_shade_params (ffi.ShadeParams)."""
        return ffi.ShadeParams(max_depth, integrator, background, ffi.F3(*background_color), 0, 0)

    def shade_hits(self, rays, hits, states, max_depth=50, integrator=ffi.VK_INTEGRATOR_PDF, background=ffi.VK_BACKGROUND_SOLID,
                   background_color=(0.0, 0.0, 0.0), out=None, return_stats=False):
        """One bounce of ray_color for caller-supplied (ray, hit, path state) items (vk_shade_hits): a SHADED_DTYPE array, out[i] the
        next ray, the state after the bounce, the status (ffi.VK_SHADE_*) and the lobe sampled for (rays[i], hits[i], states[i]).  rays
        as for trace_rays(), hits as trace_rays() returns them, states a PATH_STATE_DTYPE array (make_path_states()); host memory (the
        call has no device-pointer variant yet)."""
        sp = self.shade_params(max_depth, integrator, background, background_color)
        stats = ffi.Stats()
        rays = self._host_rays(rays)
        n = rays.shape[0]
        hits = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
        states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
        assert hits.shape[0] == n and states.shape[0] == n
        if out is None:
            out = np.zeros(n, SHADED_DTYPE)
        assert out.dtype == SHADED_DTYPE and out.flags.c_contiguous and out.shape == (n,)
        ptr = lambda a: C.c_void_p(a.ctypes.data if n else None)
        check(self._lib, self._lib.vk_shade_hits(self._h, C.byref(sp), ptr(rays), ptr(hits), ptr(states), n, ptr(out), C.byref(stats)))
        return (out, stats) if return_stats else out

    def wavefront_radiance(self, rays, seed=0, first_index=0, sample=0, max_depth=50, integrator=ffi.VK_INTEGRATOR_PDF,
                           background=ffi.VK_BACKGROUND_SOLID, background_color=(0.0, 0.0, 0.0), return_bounces=False):
        """The loop of vk_shade_hits' contract: trace_rays() and shade_hits() in turn from fresh path states until no path is left.  An
        (n, 4) float32 array: [:, :3] the radiance of sample `sample` of every ray, [:, 3] its stream's final counter (bit pattern) —
        in a scene without media what debug_radiance_samples() returns for that sample, bit for bit.  return_bounces: also the list of
        per-bounce records of wavefront_loop(), each with the two calls' stats."""
        rays = self._host_rays(rays)
        stats = []

        def trace(r, s, fi):
            hits, st = self.trace_rays(r, seed=s, first_index=fi, return_stats=True)
            stats.append({"trace": st})
            return hits

        def shade(r, h, s):
            out, st = self.shade_hits(r, h, s, max_depth, integrator, background, background_color, return_stats=True)
            stats[-1]["shade"] = st
            return out

        final, bounces = wavefront_loop(trace, shade, rays, make_path_states(rays.shape[0], seed, first_index, sample), seed, first_index)
        res = np.zeros((rays.shape[0], 4), np.float32)
        res[:, :3] = final["acc"]
        res[:, 3] = np.ascontiguousarray(final["counter"]).view(np.float32)
        if return_bounces:
            for b, st in zip(bounces, stats):
                b.update(st)
            return res, bounces
        return res

    def debug_radiance_samples(self, rays, keys=None, return_stats=False, **params):
        """Every sample of trace_radiance() (vk_debug_trace_radiance_samples, a test hook): an (n, samples_per_ray, 4) float32 array,
        [..., :3] the radiance before the finite filter, [..., 3] the stream's final counter (bit pattern).  keys: None, or one
        (seed, pixel, sample, ctr) per ray as a KEY_DTYPE array, whose streams the samples resume.  params: radiance_params()'s keywords."""
        rp = self.radiance_params(**params)
        stats = ffi.Stats()
        rays = self._host_rays(rays)
        n = rays.shape[0]
        if keys is not None:
            keys = np.ascontiguousarray(keys, KEY_DTYPE).reshape(-1)
            assert keys.shape[0] == n
        out = np.zeros((n, rp.samples_per_ray, 4), np.float32)
        self._host_batch("vk_debug_trace_radiance_samples", rp, stats, rays, keys, out)
        return (out, stats) if return_stats else out

    def trace_irradiance(self, points, seed=0, first_index=0, samples_per_ray=1, first_sample=0, max_depth=50,
                         integrator=ffi.VK_INTEGRATOR_PDF, background=ffi.VK_BACKGROUND_SOLID, background_color=(0.0, 0.0, 0.0), out=None,
                         return_stats=False):
        """Cosine-weighted mean radiance arriving at caller-supplied surface points (vk_trace_irradiance): an (n, 3) float32 array,
        out[i] the mean of samples first_sample .. first_sample + samples_per_ray - 1 of points[i], each a direction drawn on the device
        around the point's normal and ray_color along it on the same stream.  Irradiance is pi * out; a Lambertian texel of albedo a
        radiates a * out.  points: make_points() / points_from_hits() (host memory; the call has no device-pointer variant yet)."""
        rp = self.radiance_params(seed, first_index, samples_per_ray, first_sample, max_depth, integrator, background, background_color)
        stats = ffi.Stats()
        points = self._host_rays(points)
        n = points.shape[0]
        if out is None:
            out = np.zeros((n, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (n, 3)
        self._host_batch("vk_trace_irradiance", rp, stats, points, out)
        return (out, stats) if return_stats else out

    def debug_irradiance_samples(self, points, return_stats=False, **params):
        """Every sample of trace_irradiance() (vk_debug_trace_irradiance_samples, a test hook): (samples, dirs), both
        (n, samples_per_ray, 4) float32 — samples[..., :3] the radiance before the finite filter, samples[..., 3] the stream's final
        counter (bit pattern), dirs[..., :3] the direction drawn for the sample.  params: radiance_params()'s keywords."""
        rp = self.radiance_params(**params)
        stats = ffi.Stats()
        points = self._host_rays(points)
        n = points.shape[0]
        samples = np.zeros((n, rp.samples_per_ray, 4), np.float32)
        dirs = np.zeros((n, rp.samples_per_ray, 4), np.float32)
        self._host_batch("vk_debug_trace_irradiance_samples", rp, stats, points, samples, dirs)
        return (samples, dirs, stats) if return_stats else (samples, dirs)

    def trace_probes(self, probes, seed=0, first_index=0, samples_per_ray=1, first_sample=0, max_depth=50,
                     integrator=ffi.VK_INTEGRATOR_PDF, background=ffi.VK_BACKGROUND_SOLID, background_color=(0.0, 0.0, 0.0), out=None,
                     return_stats=False):
        """Spherical-harmonic light probes at caller-supplied points (vk_trace_probes): an (n, 9, 3) float32 array, out[i, k, c] the mean
        over samples first_sample .. first_sample + samples_per_ray - 1 of probes[i] of Y_k(u) * L_c(u), each a uniform direction u drawn
        on the device and ray_color along it on the same stream.  The radiance's SH coefficient is 4 pi * out; probe_eval() answers for a
        normal.  probes: make_probes() (host memory; the call has no device-pointer variant yet)."""
        rp = self.radiance_params(seed, first_index, samples_per_ray, first_sample, max_depth, integrator, background, background_color)
        stats = ffi.Stats()
        probes = self._host_rays(probes)
        n = probes.shape[0]
        if out is None:
            out = np.zeros((n, ffi.VK_PROBE_COEFFS, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (n, ffi.VK_PROBE_COEFFS, 3)
        self._host_batch("vk_trace_probes", rp, stats, probes, out)
        return (out, stats) if return_stats else out

    def debug_probe_samples(self, probes, return_stats=False, **params):
        """Every sample of trace_probes() (vk_debug_trace_probe_samples, a test hook): (samples, dirs), both (n, samples_per_ray, 4)
        float32 — samples[..., :3] the radiance before the finite filter, samples[..., 3] the stream's final counter (bit pattern),
        dirs[..., :3] the unit direction drawn for the sample.  params: radiance_params()'s keywords."""
        rp = self.radiance_params(**params)
        stats = ffi.Stats()
        probes = self._host_rays(probes)
        n = probes.shape[0]
        samples = np.zeros((n, rp.samples_per_ray, 4), np.float32)
        dirs = np.zeros((n, rp.samples_per_ray, 4), np.float32)
        self._host_batch("vk_debug_trace_probe_samples", rp, stats, probes, samples, dirs)
        return (samples, dirs, stats) if return_stats else (samples, dirs)

    GUIDE_CHANNELS = AOV_CHANNELS + ("bounces",)

    def guide_params(self, **overrides):
        """The library's default vk_guide_params (max_bounces 4, fuzz_max 0), with fields overridden by keyword."""
        gp = ffi.GuideParams()
        check(self._lib, self._lib.vk_guide_default_params(C.byref(gp)))
        for k, v in overrides.items():
            if k not in dict(ffi.GuideParams._fields_):
                raise ValueError(f"unknown vk_guide_params field {k!r}")
            setattr(gp, k, v)
        return gp

    def render_guides(self, cam, params, first_sample=0, guide=None, want=GUIDE_CHANNELS, out=None):
        """Specular guides of samples [first_sample, first_sample + params.samples_per_pixel) (vk_render_guides): render_aov()'s
        buffers followed through mirrors and glass to the first rough surface, plus 'bounces' (height, width), the mean number of
        continuations.  guide: a vk_guide_params (guide_params()), default = the library's.  Returns (dict, vk_stats)."""
        want = tuple(want)
        unknown = set(want) - set(self.GUIDE_CHANNELS)
        if unknown or not want:
            raise ValueError(f"want must be a non-empty subset of {self.GUIDE_CHANNELS}, got {want}")
        gp = guide if guide is not None else self.guide_params()
        bufs = dict(out or {})
        for ch in want:
            shape = (params.height, params.width, 3) if ch in ("albedo", "normal") else (params.height, params.width)
            if ch not in bufs:
                bufs[ch] = np.zeros(shape, dtype=np.float32)
            assert bufs[ch].dtype == np.float32 and bufs[ch].flags.c_contiguous
        ptrs = [C.c_void_p(bufs[ch].ctypes.data) if ch in want else None for ch in self.GUIDE_CHANNELS]
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_render_guides(self._h, C.byref(cam), C.byref(params), first_sample, C.byref(gp), *ptrs,
                                                    C.byref(stats)))
        return {ch: bufs[ch] for ch in want}, stats

    def render_guides_device(self, cam, params, first_sample, guide=None, d_albedo=0, d_normal=0, d_depth=0, d_coverage=0, d_bounces=0,
                             stream=None):
        """Enqueue the specular guides into device memory (vk_render_guides_device, no host sync); a 0 pointer = not wanted."""
        gp = guide if guide is not None else self.guide_params()
        stats = ffi.Stats()
        ptrs = [C.c_void_p(p or None) for p in (d_albedo, d_normal, d_depth, d_coverage, d_bounces)]
        check(self._lib, self._lib.vk_render_guides_device(self._h, C.byref(cam), C.byref(params), first_sample, C.byref(gp), *ptrs,
                                                           C.c_void_p(stream or 0), C.byref(stats)))
        return stats

    def render_mattes(self, cam, params, first_sample=0, kind=ffi.VK_MATTE_OBJECT, ranks=6, overflow=True, out=None, return_stats=False):
        """ID mattes of samples [first_sample, first_sample + params.samples_per_pixel) (vk_render_mattes): which object (kind
        VK_MATTE_OBJECT: a vk_ref as trace_rays() names it) or which material (VK_MATTE_MATERIAL) the primary rays of each pixel show,
        VK_MATTE_BACKGROUND for a miss.  Returns uint32 arrays, y = 0 the bottom row: ids and counts (height, width, ranks), sorted by
        count descending, unused slots (0, 0), and overflow (height, width) — the samples that found the table full — or None with
        overflow=False.  out: (ids, counts, overflow) to write into (pixels outside this call's tile partition keep their values)."""
        shape = (params.height, params.width)
        ids, counts, over = out if out is not None else (np.zeros(shape + (ranks,), np.uint32), np.zeros(shape + (ranks,), np.uint32),
                                                        np.zeros(shape, np.uint32) if overflow else None)
        assert _matte_table(ids, counts, over) == (ranks, params.height * params.width)
        mp = ffi.MatteParams()
        check(self._lib, self._lib.vk_matte_default_params(C.byref(mp)))
        mp.kind, mp.ranks = kind, ranks
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_render_mattes(self._h, C.byref(cam), C.byref(params), first_sample, C.byref(mp),
                                                    C.c_void_p(ids.ctypes.data), C.c_void_p(counts.ctypes.data),
                                                    C.c_void_p(over.ctypes.data) if over is not None else None, C.byref(stats)))
        return (ids, counts, over, stats) if return_stats else (ids, counts, over)

    def debug_matte_samples(self, cam, params, first_sample=0, kind=ffi.VK_MATTE_OBJECT, out=None):
        """vk_debug_matte_samples: the id of every sample render_mattes() would count, (height, width, samples_per_pixel) uint32"""
        if out is None:
            out = np.zeros((params.height, params.width, params.samples_per_pixel), np.uint32)
        assert out.dtype == np.uint32 and out.flags.c_contiguous
        check(self._lib, self._lib.vk_debug_matte_samples(self._h, C.byref(cam), C.byref(params), first_sample, kind,
                                                          C.c_void_p(out.ctypes.data)))
        return out

    def denoise_params(self, width, height, **overrides):
        """vk_denoise_default_params for a width x height image, with fields overridden by keyword (levels=, sigma_l=, ...)"""
        dp = ffi.DenoiseParams()
        check(self._lib, self._lib.vk_denoise_default_params(width, height, C.byref(dp)))
        for k, v in overrides.items():
            if k not in dict(ffi.DenoiseParams._fields_):
                raise ValueError(f"unknown vk_denoise_params field {k!r}")
            setattr(dp, k, v)
        return dp

    def denoise(self, color, stderr=None, albedo=None, normal=None, depth=None, params=None, out=None):
        """Denoise a frame (vk_denoise): color (height, width, 3) float32 with y = 0 the bottom row, as render() gives it; the optional
        guides in the same layout — stderr (Progress.stderr()), albedo and normal (height, width, 3), depth (height, width), as
        render_aov() gives them; None switches a guide's term off.  params: a vk_denoise_params (denoise_params()), default = the
        library's defaults for this size.  Returns (image, vk_stats)."""
        h, w = color.shape[:2]
        dp = params if params is not None else self.denoise_params(w, h)
        if out is None:
            out = np.zeros((h, w, 3), np.float32)
        ptrs = []
        for a, shape in ((color, (h, w, 3)), (stderr, (h, w, 3)), (albedo, (h, w, 3)), (normal, (h, w, 3)), (depth, (h, w)), (out, (h, w, 3))):
            if a is not None:
                assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == shape, (a.dtype, a.shape, shape)
            ptrs.append(C.c_void_p(a.ctypes.data) if a is not None else None)
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_denoise(self._h, C.byref(dp), *ptrs, C.byref(stats)))
        return out, stats

    def denoise_device(self, params, d_color, d_out, d_stderr=0, d_albedo=0, d_normal=0, d_depth=0, stream=None):
        """Enqueue the denoiser on device buffers (vk_denoise_device, no host sync); a 0 pointer switches a guide's term off."""
        check(self._lib, self._lib.vk_denoise_device(self._h, C.byref(params), C.c_void_p(d_color), C.c_void_p(d_stderr or None),
                                                     C.c_void_p(d_albedo or None), C.c_void_p(d_normal or None),
                                                     C.c_void_p(d_depth or None), C.c_void_p(d_out), C.c_void_p(stream or 0)))

    def render_device(self, cam, params, d_ptr, stream=None):
        """Enqueue a render into device memory at d_ptr on `stream` (no host sync)."""
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_render_device(self._h, C.byref(cam), C.byref(params), C.c_void_p(d_ptr),
                                                    C.c_void_p(stream or 0), C.byref(stats)))
        return stats

    def last_kernel_ms(self):
        """HIP-event time of the launches of the last render (waits for them)."""
        ms = C.c_double()
        check(self._lib, self._lib.vk_scene_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def parts(self):
        """one record per device share of the scene (vk_scene_part_info): device, name, PCI bus id, peer access to devices[0], the kernel
        time of its launches in the last frame (waits for them)"""
        out = []
        pi = ffi.PartInfo()
        check(self._lib, self._lib.vk_scene_part_info(self._h, 0, C.byref(pi)))
        for j in range(pi.n_parts):
            check(self._lib, self._lib.vk_scene_part_info(self._h, j, C.byref(pi)))
            out.append({"part": j, "device_index": pi.device, "device": pi.name.decode(), "pci_bus_id": pi.pci_bus_id.decode(),
                        "can_access_devices0": bool(pi.can_access_landing_device), "kernel_ms": round(pi.kernel_ms, 3)})
        return out

    def last_requeued_samples(self):
        """Exact re-treeing: samples of the last render that went through the second launch, on the tree as handed over (waits)."""
        n = C.c_uint64()
        check(self._lib, self._lib.vk_scene_last_requeued_samples(self._h, C.byref(n)))
        return n.value

    def pack_tiles_device(self, d_fb, width, height, output_format, tile_rank, tile_world, d_slab, stream=None):
        """this rank's tiles of the f32 framebuffer at d_fb -> its slab at d_slab (floats, or bytes through to_color for RGB8)"""
        check(self._lib, self._lib.vk_pack_tiles_device(self._h, C.c_void_p(d_fb), width, height, output_format, tile_rank, tile_world,
                                                        C.c_void_p(d_slab), C.c_void_p(stream or 0)))

    def unpack_tiles_device(self, d_slab, width, height, output_format, tile_rank, tile_world, d_img, stream=None):
        """rank tile_rank's slab at d_slab -> its tiles of the full image at d_img (f32 y up, or RGB8 top row first)"""
        check(self._lib, self._lib.vk_unpack_tiles_device(self._h, C.c_void_p(d_slab), width, height, output_format, tile_rank, tile_world,
                                                          C.c_void_p(d_img), C.c_void_p(stream or 0)))

    def progress(self, cam, params, stderr=False, adaptive=None):
        """A progressive render of ONE frame (vk_progress_create): params.samples_per_pixel is the budget, step(n) renders the next n
        samples per pixel and returns the running mean — bit for bit the image render() gives at samples_per_pixel = samples done.
        adaptive=dict(abs_tol=, rel_tol=, min_samples=, min_steps=): converged tiles stop (Progress.set_adaptive; implies stderr)."""
        pr = Progress(self, cam, params, stderr or adaptive is not None)
        if adaptive is not None:
            try:
                pr.set_adaptive(**adaptive)
            except Exception:
                pr.close()
                raise
        return pr

    def temporal(self, width, height, **overrides):
        """A temporal accumulator for width x height frames of this scene (vk_temporal_create): the library's default parameters with
        fields overridden by keyword (max_history=, depth_tol=, normal_cos_min=, albedo_floor=).  Use as a context manager, or close()."""
        tp = ffi.TemporalParams()
        check(self._lib, self._lib.vk_temporal_default_params(width, height, C.byref(tp)))
        for k, v in overrides.items():
            if k not in dict(ffi.TemporalParams._fields_):
                raise ValueError(f"unknown vk_temporal_params field {k!r}")
            setattr(tp, k, v)
        return Temporal(self, tp)

    def paths(self, capacity):
        """A path batch of up to `capacity` paths on this scene (vk_paths_create): the loop of wavefront_radiance() on the device, with
        a stable compaction of the survivors per bounce.  Use as a context manager, or close() it before the scene."""
        return PathBatch(self, capacity)

    def film(self, cam, params):
        """A film on this scene (vk_film_create): a frame's fixed-point sums with its camera and render parameters, which emits camera
        paths into a path batch and deposits finished batches, both on the device.  Use as a context manager, or close() it before the
        scene."""
        return Film(self, cam, params)

    def splat(self, width, height, spp, filter=ffi.VK_SPLAT_MITCHELL, radius=2.0, b=1.0 / 3.0, c=1.0 / 3.0):
        """A filtered accumulator on this scene (vk_splat_create): per pixel the sums of r, g, b and of the reconstruction filter's
        weight, into which finished path batches are splatted on the device.  filter: ffi.VK_SPLAT_BOX, _TENT or _MITCHELL (b, c); radius
        in pixels, 0.5 .. 2.  Use as a context manager, or close() it before the scene."""
        return Splat(self, width, height, spp, ffi.SplatParams(filter, radius, b, c))

    def robust(self, width, height, spp, buckets=8, mode=ffi.VK_ROBUST_GINI, trim=0):
        """A robust accumulator on this scene (vk_robust_create): per pixel `buckets` partial sums of r, g, b and a count, into which
        finished path batches are deposited on the device (sample s of a pixel into bucket s % buckets), resolved as the plain mean
        (ffi.VK_ROBUST_MEAN), the mean without `trim` buckets per side (_TRIM) or without as many as the buckets' Gini coefficient asks
        for (_GINI).  Use as a context manager, or close() it before the scene."""
        return Robust(self, width, height, spp, ffi.RobustParams(buckets, mode, trim, 0))

    def lpe(self, width, height, spp, capacity, rules=None, n_layers=None, rest_layer=None):
        """Light-path layers on this scene (vk_lpe_create): a tracker that steps path batches of up to `capacity` paths as
        PathBatch.step() does while keeping a tag of every path's bounces, and per pixel and layer the sums of r, g, b and a count, into
        which finished batches are deposited by the first matching rule.  rules: a list of lpe_rule() values with n_layers and
        rest_layer; None: standard_rules(), whose layers are STANDARD_LAYERS.  Use as a context manager, or close() it before the
        scene."""
        if rules is None:
            rules = standard_rules()
            n_layers = len(STANDARD_LAYERS) if n_layers is None else n_layers
            rest_layer = STANDARD_LAYERS.index("rest") if rest_layer is None else rest_layer
        return LightPathLayers(self, width, height, spp, capacity, rules, n_layers, 0 if rest_layer is None else rest_layer)

    def tone(self, width, height):
        """A display transform on this scene's device (vk_tone_create) for frames of width x height: auto-exposure from a luminance
        histogram, a tone curve (clamp, Reinhard, Hable, ACES) and a transfer (the reference's, sRGB, gamma 2.2; optionally dithered) to
        8-bit codes.  Use as a context manager, or close() it before the scene."""
        return Tone(self, width, height)

    def nlm(self, width, height):
        """A non-local-means filter on this scene's device (vk_nlm_create) for frames of width x height: a frame and its standard error
        in, the filtered frame and its propagated standard error out; the weights come from the colour image and its variance alone.  Use
        as a context manager, or close() it before the scene."""
        return NonLocalMeans(self, width, height)

    def glare(self, width, height):
        """A glare stage on this scene's device (vk_glare_create) for frames of width x height: a float frame in, the frame with the
        share `strength` of its bright part spread over a pyramid of halved images out, for Tone.load / load_device.  Use as a context
        manager, or close() it before the scene."""
        return Glare(self, width, height)

    def psf(self, width, height, kmax):
        """A point-spread stage on this scene's device (vk_psf_create) for frames of width x height and kernels up to kmax x kmax: a
        float frame in, the frame convolved with the loaded kernel out, between glare() and tone().  Close it before the scene."""
        return Psf(self, width, height, kmax)

    def upsample(self, w, h, W, H):
        """A guided upsampler on this scene's device (vk_upsample_create) from w x h to W x H: load() a low frame with its stderr3 and
        first-hit buffers, apply() with the first-hit buffers at the high size.  Use as a context manager, or close() it before the
        scene."""
        return Upsample(self, w, h, W, H)

    def debug_compact_paths(self, items, ids, n_ids, canary=0xA5, roulette=None):
        """The compaction of a path batch's bounce on host arrays (vk_debug_compact_paths, a test hook): items a SHADED_DTYPE array, ids
        their uint32 ids (each below n_ids).  Every output is prefilled with the byte `canary`.  Returns (rays, states, ids_out — n
        entries each, the survivors first —, result_state, result_status — n_ids entries —, counts by status).  roulette = (first_depth,
        q_min, q_max): the compaction with that termination rule in its count pass (vk_debug_compact_roulette)."""
        items = np.ascontiguousarray(items, SHADED_DTYPE).reshape(-1)
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        n = items.shape[0]
        assert ids.shape[0] == n
        outs = [np.zeros(n, RAY_DTYPE), np.zeros(n, PATH_STATE_DTYPE), np.zeros(n, np.uint32), np.zeros(n_ids, PATH_STATE_DTYPE),
                np.zeros(n_ids, np.uint32)]
        for a in outs:
            a.view(np.uint8)[:] = canary
        counts = (C.c_uint64 * 5)()
        ptr = lambda a: C.c_void_p(a.ctypes.data if a.size else None)
        tail = (ptr(items), ptr(ids), n, n_ids, *[C.c_void_p(a.ctypes.data) for a in outs], C.byref(counts))
        if roulette is None:
            check(self._lib, self._lib.vk_debug_compact_paths(self._h, *tail))
        else:
            check(self._lib, self._lib.vk_debug_compact_roulette(self._h, C.byref(ffi.RouletteParams(*roulette, 0)), *tail))
        return (*outs, np.array(list(counts), np.uint64))

    def to_color_device(self, d_rgb, width, height, d_rgb8, stream=None):
        check(self._lib, self._lib.vk_to_color_device(self._h, C.c_void_p(d_rgb), width, height, C.c_void_p(d_rgb8), C.c_void_p(stream or 0)))

    def close(self):
        if self._h:
            self._lib.vk_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Progress:
    """vk_progress handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed)."""

    def __init__(self, scene, cam, params, stderr=False):
        self._lib = scene._lib
        self._scene = scene
        self.params = params
        h = C.c_void_p()
        check(self._lib, self._lib.vk_progress_create(scene._h, C.byref(cam), C.byref(params),
                                                      ffi.VK_PROGRESS_STDERR if stderr else 0, C.byref(h)))
        self._h = h

    def step(self, n, out=None):
        """Render the next n samples per pixel; returns (image, vk_stats of the window): float32 (height, width, 3) with y = 0 the bottom
        row, or uint8 with row 0 the top row (VK_OUTPUT_RGB8).  Only this partition's pixels of `out` are written."""
        p = self.params
        dt = np.uint8 if p.output_format == ffi.VK_OUTPUT_RGB8 else np.float32
        if out is None:
            out = np.zeros((p.height, p.width, 3), dtype=dt)
        assert out.dtype == dt and out.flags.c_contiguous and out.size == p.width * p.height * 3
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_progress_step(self._h, n, out.ctypes.data_as(C.c_void_p), C.byref(stats)))
        return out, stats

    def step_device(self, n, d_ptr, stream=None):
        """Enqueue the next n samples per pixel; the running mean goes to device memory at d_ptr on `stream` (no host sync)."""
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_progress_step_device(self._h, n, C.c_void_p(d_ptr), C.c_void_p(stream or 0), C.byref(stats)))
        return stats

    def stderr(self):
        """Batch-means standard error of the running mean, float32 (height, width, 3), y = 0 the bottom row (needs stderr=True and two
        steps or more)."""
        p = self.params
        out = np.zeros((p.height, p.width, 3), np.float32)
        check(self._lib, self._lib.vk_progress_stderr(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def stderr_device(self, d_ptr, stream=None):
        """stderr() into device memory at d_ptr (vk_progress_stderr_device: width*height*3 floats, this partition's pixels only), enqueued
        on `stream`; bit-identical to stderr().  Not for handles on a multi-device scene."""
        check(self._lib, self._lib.vk_progress_stderr_device(self._h, C.c_void_p(d_ptr), C.c_void_p(stream or 0)))

    def set_adaptive(self, abs_tol=0.0, rel_tol=0.0, min_samples=0, min_steps=2):
        """Adaptive sampling (vk_progress_set_adaptive): after every window a tile whose pixels all have, per component,
        stderr <= abs_tol + rel_tol * |mean| (and min_samples samples, min_steps windows) is frozen; before the first step."""
        ap = ffi.AdaptiveParams(abs_tol, rel_tol, min_samples, min_steps)
        check(self._lib, self._lib.vk_progress_set_adaptive(self._h, C.byref(ap)))

    def tile_samples(self):
        """(samples per tile as uint32 (tiles_y, tiles_x), tile row 0 at the bottom and 0 outside the partition; vk_adaptive_info)"""
        p = self.params
        out = np.zeros(((p.height + 7) // 8, (p.width + 7) // 8), np.uint32)
        inf = ffi.AdaptiveInfo()
        check(self._lib, self._lib.vk_progress_tile_samples(self._h, out.ctypes.data_as(C.c_void_p), C.byref(inf)))
        return out, inf

    def moments(self):
        """(running fixed-point sums as int64, error moments as float64 or None), each (height, width, 3) y up: vk_debug_progress_moments"""
        p = self.params
        run = np.zeros((p.height, p.width, 3), np.int64)
        m2 = np.zeros((p.height, p.width, 3), np.float64) if self.info().flags & ffi.VK_PROGRESS_STDERR else None
        check(self._lib, self._lib.vk_debug_progress_moments(self._h, run.ctypes.data_as(C.c_void_p),
                                                             m2.ctypes.data_as(C.c_void_p) if m2 is not None else None))
        return run, m2

    def info(self):
        inf = ffi.ProgressInfo()
        check(self._lib, self._lib.vk_progress_get_info(self._h, C.byref(inf)))
        return inf

    def reset(self, cam=None):
        """Back to sample 0, with a new camera or the same one."""
        check(self._lib, self._lib.vk_progress_reset(self._h, C.byref(cam) if cam is not None else None))

    def close(self):
        if self._h:
            self._lib.vk_progress_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Temporal:
    """vk_temporal handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed)."""

    def __init__(self, scene, params):
        self._lib = scene._lib
        self._scene = scene
        self.params = params
        h = C.c_void_p()
        check(self._lib, self._lib.vk_temporal_create(scene._h, C.byref(params), C.byref(h)))
        self._h = h

    def accumulate(self, cam, color, normal, depth, stderr=None, albedo=None, want_history=False):
        """Blend a frame into the history (vk_temporal_accumulate): color and normal (height, width, 3) float32 with y = 0 the bottom
        row, depth (height, width), as render() and render_aov() give them, under the camera `cam`; stderr (Progress.stderr()) and
        albedo are optional.  Returns (color, stderr or None, history length per pixel or None, vk_stats): the first two are what
        DeviceScene.denoise() takes."""
        h, w = self.params.height, self.params.width
        out = np.zeros((h, w, 3), np.float32)
        out_se = np.zeros((h, w, 3), np.float32) if stderr is not None else None
        out_n = np.zeros((h, w), np.float32) if want_history else None
        ptrs = []
        for a, shape in ((color, (h, w, 3)), (stderr, (h, w, 3)), (albedo, (h, w, 3)), (normal, (h, w, 3)), (depth, (h, w)),
                         (out, (h, w, 3)), (out_se, (h, w, 3)), (out_n, (h, w))):
            if a is not None:
                assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == shape, (a.dtype, a.shape, shape)
            ptrs.append(C.c_void_p(a.ctypes.data) if a is not None else None)
        stats = ffi.Stats()
        check(self._lib, self._lib.vk_temporal_accumulate(self._h, C.byref(cam), *ptrs, C.byref(stats)))
        return out, out_se, out_n, stats

    def accumulate_device(self, cam, d_color, d_normal, d_depth, d_out_color, d_stderr=0, d_albedo=0, d_out_stderr=0, d_out_history=0,
                          stream=None):
        """Enqueue a frame on device buffers (vk_temporal_accumulate_device, no host sync); a 0 pointer = not given / not wanted."""
        check(self._lib, self._lib.vk_temporal_accumulate_device(
            self._h, C.byref(cam), C.c_void_p(d_color), C.c_void_p(d_stderr or None), C.c_void_p(d_albedo or None), C.c_void_p(d_normal),
            C.c_void_p(d_depth), C.c_void_p(d_out_color), C.c_void_p(d_out_stderr or None), C.c_void_p(d_out_history or None),
            C.c_void_p(stream or 0)))

    def reset(self):
        """Forget the history: the next frame is a first frame."""
        check(self._lib, self._lib.vk_temporal_reset(self._h))

    def info(self):
        inf = ffi.TemporalInfo()
        check(self._lib, self._lib.vk_temporal_get_info(self._h, C.byref(inf)))
        return inf

    def close(self):
        if self._h:
            self._lib.vk_temporal_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PathBatch:
    """vk_paths handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): begin() a batch of rays and
    path states, step() it bounce by bounce on the device, read() or cull() the live paths between steps, results() at any time."""

    def __init__(self, scene, capacity):
        self._lib = scene._lib
        self._scene = scene
        h = C.c_void_p()
        check(self._lib, self._lib.vk_paths_create(scene._h, capacity, C.byref(h)))
        self._h = h

    def begin(self, rays, states, max_depth=50, integrator=ffi.VK_INTEGRATOR_PDF, background=ffi.VK_BACKGROUND_SOLID,
              background_color=(0.0, 0.0, 0.0)):
        """Start a batch (vk_paths_begin): path i has the id i, rays[i] (a RAY_DTYPE array) and states[i] (a PATH_STATE_DTYPE array,
        make_path_states()); the keywords are DeviceScene.shade_params()'s.  Forgets the handle's previous batch."""
        sp = DeviceScene.shade_params(max_depth, integrator, background, background_color)
        rays = DeviceScene._host_rays(rays)
        states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
        n = rays.shape[0]
        assert states.shape[0] == n
        ptr = lambda a: C.c_void_p(a.ctypes.data if n else None)
        check(self._lib, self._lib.vk_paths_begin(self._h, C.byref(sp), ptr(rays), ptr(states), n))

    def step(self, max_bounces=1):
        """Run bounces until nothing is live or max_bounces are run (vk_paths_step): the call's ffi.PathsStepInfo."""
        info = ffi.PathsStepInfo()
        check(self._lib, self._lib.vk_paths_step(self._h, max_bounces, C.byref(info)))
        return info

    def run(self):
        """step() until nothing is live: the list of the calls' ffi.PathsStepInfo, one bounce each."""
        out = []
        while self.info().live:
            out.append(self.step(1))
        return out

    def read(self):
        """The live paths in live order (vk_paths_read): (ids uint32, rays RAY_DTYPE, states PATH_STATE_DTYPE)."""
        n = int(self.info().live)
        ids, rays, states = np.zeros(n, np.uint32), np.zeros(n, RAY_DTYPE), np.zeros(n, PATH_STATE_DTYPE)
        ptr = lambda a: C.c_void_p(a.ctypes.data if n else None)
        check(self._lib, self._lib.vk_paths_read(self._h, ptr(ids), ptr(rays), ptr(states)))
        return ids, rays, states

    def cull(self, keep, scale=None):
        """Retire the live paths whose keep byte is 0 as ffi.VK_PATHS_CULLED and multiply the kept ones' throughput by scale (one float
        per live path) where that is given (vk_paths_cull); both in live order."""
        n = int(self.info().live)
        keep = np.ascontiguousarray(keep, np.uint8).reshape(-1)
        assert keep.shape[0] == n
        if scale is not None:
            scale = np.ascontiguousarray(scale, np.float32).reshape(-1)
            assert scale.shape[0] == n
        check(self._lib, self._lib.vk_paths_cull(self._h, C.c_void_p(keep.ctypes.data if n else None),
                                                 C.c_void_p(scale.ctypes.data) if scale is not None and n else None))

    def set_roulette(self, first_depth, q_min=None, q_max=None):
        """The handle's termination rule (vk_roulette_set): from the next bounce on, every bounce of step() and of Film.regen_step()
        ends a scattered path of state.depth >= first_depth with probability 1 - q, q = its largest throughput component clamped to
        [q_min, q_max], and scales a continuing one's throughput by 1 / q — on the device, inside the compaction.  set_roulette(None)
        turns the rule off.  It is the handle's: begin(), Film.emit() and Film.regen_begin() keep it."""
        if first_depth is None:
            check(self._lib, self._lib.vk_roulette_set(self._h, None))
        else:
            check(self._lib, self._lib.vk_roulette_set(self._h, C.byref(ffi.RouletteParams(first_depth, q_min, q_max, 0))))

    def roulette(self):
        """(first_depth, q_min, q_max) of the rule that is set, or None (vk_roulette_get)"""
        rp, on = ffi.RouletteParams(), C.c_int()
        check(self._lib, self._lib.vk_roulette_get(self._h, C.byref(rp), C.byref(on)))
        return (rp.first_depth, rp.q_min, rp.q_max) if on.value else None

    def results(self):
        """Per started id the final (or, for a live path, current) state and the status (vk_paths_results): (PATH_STATE_DTYPE array,
        uint32 array of ffi.VK_SHADE_* / ffi.VK_PATHS_*)."""
        n = int(self.info().started)
        states, status = np.zeros(n, PATH_STATE_DTYPE), np.zeros(n, np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data if n else None)
        check(self._lib, self._lib.vk_paths_results(self._h, ptr(states), ptr(status)))
        return states, status

    def radiance(self):
        """results() in debug_radiance_samples()' form: an (n, 4) float32 array, [:, :3] acc and [:, 3] the counter's bit pattern"""
        states, _ = self.results()
        res = np.zeros((states.shape[0], 4), np.float32)
        res[:, :3] = states["acc"]
        res[:, 3] = np.ascontiguousarray(states["counter"]).view(np.float32)
        return res

    def last_ms(self):
        """(trace, shade, compaction) device milliseconds of the last bounce (vk_debug_paths_last_ms, a test hook)"""
        ms = (C.c_double * 3)()
        check(self._lib, self._lib.vk_debug_paths_last_ms(self._h, C.byref(ms)))
        return tuple(ms)

    def info(self):
        inf = ffi.PathsInfo()
        check(self._lib, self._lib.vk_paths_get_info(self._h, C.byref(inf)))
        return inf

    def close(self):
        if self._h:
            self._lib.vk_paths_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Film:
    """vk_film handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): emit() camera paths of a
    window of the frame into a PathBatch, step the batch to its end, deposit() it; resolve() once every sample went through is render()'s
    frame, bit for bit."""

    def __init__(self, scene, cam, params):
        self._lib = scene._lib
        self._scene = scene
        self.params = ffi.RenderParams.from_buffer_copy(params)
        h = C.c_void_p()
        check(self._lib, self._lib.vk_film_create(scene._h, C.byref(cam), C.byref(params), C.byref(h)))
        self._h = h

    def emit(self, batch, x0, y0, w, h, first_sample=0, n_samples=1):
        """Begin `batch` with the w * h * n_samples camera paths of the window (vk_film_emit): id ((y - y0) * w + (x - x0)) * n_samples + k
        is sample first_sample + k of pixel (x, y)."""
        win = ffi.FilmWindow(x0, y0, w, h, first_sample, n_samples)
        check(self._lib, self._lib.vk_film_emit(self._h, batch._h, C.byref(win)))

    def deposit(self, batch):
        """Add the retired paths of `batch`, which has nothing live, to the frame's sums (vk_film_deposit), each at its state's pixel."""
        check(self._lib, self._lib.vk_film_deposit(self._h, batch._h))

    def resolve(self, n=None, out=None):
        """The frame as the mean over n samples per pixel (vk_film_resolve; default: the film's samples_per_pixel): float32 (height,
        width, 3), y = 0 the bottom row.  out: an array of that shape to write into."""
        p = self.params
        if out is None:
            out = np.zeros((p.height, p.width, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == p.width * p.height * 3
        check(self._lib, self._lib.vk_film_resolve(self._h, p.samples_per_pixel if n is None else n, out.ctypes.data_as(C.c_void_p)))
        return out

    def reset(self, cam=None):
        """Zero the sums and the counters; cam, where given, replaces the camera (vk_film_reset)."""
        check(self._lib, self._lib.vk_film_reset(self._h, C.byref(cam) if cam is not None else None))

    def info(self):
        inf = ffi.FilmInfo()
        check(self._lib, self._lib.vk_film_get_info(self._h, C.byref(inf)))
        return inf

    _KEEP = object()      # roulette=: leave the batch's rule as it is

    def render(self, batch, cull=None, roulette=_KEEP):
        """The whole frame through `batch`: the frame is walked in windows that fit the batch's capacity — whole rows of all samples
        where a row fits, else pieces of a row, else a pixel's samples in pieces —, each emitted, stepped to its end and deposited.
        cull, where given, is called with the batch between two bounces while anything is live (PathBatch.read() and cull() are its
        tools).  roulette, where given, is set on the batch first: (first_depth, q_min, q_max) or None (PathBatch.set_roulette).  Returns
        resolve()."""
        if roulette is not Film._KEEP:
            batch.set_roulette(*(roulette or (None,)))
        for win in self.windows(int(batch.info().capacity)):
            self.emit(batch, *win)
            while batch.step(1).live:
                if cull is not None:
                    cull(batch)
            self.deposit(batch)
        return self.resolve()

    def windows(self, capacity):
        """render()'s walk of the frame for a batch of `capacity` paths: (x0, y0, w, h, first_sample, n_samples) per window"""
        p = self.params
        cap = int(capacity)
        spp = p.samples_per_pixel
        ns = min(spp, cap)
        w = max(1, min(p.width, cap // ns))
        h = max(1, min(p.height, cap // (ns * w))) if w == p.width else 1
        for s0 in range(0, spp, ns):
            for y0 in range(0, p.height, h):
                for x0 in range(0, p.width, w):
                    yield x0, y0, min(w, p.width - x0), min(h, p.height - y0), s0, min(ns, spp - s0)

    def regen_begin(self, batch, x0, y0, w, h, first_sample=0, n_samples=1):
        """Put `batch` into its regenerating state for the window (vk_regen_begin): its w * h * n_samples paths, numbered as emit() numbers
        them, will go through the batch whatever its capacity.  Nothing is emitted yet."""
        win = ffi.FilmWindow(x0, y0, w, h, first_sample, n_samples)
        check(self._lib, self._lib.vk_regen_begin(self._h, batch._h, C.byref(win)))

    def regen_step(self, batch, max_bounces=1):
        """Run bounces of the regenerating `batch` until its run is finished or max_bounces are run (vk_regen_step): each tops the batch up
        from the window, traces, shades, deposits the retired paths into the film and compacts the survivors.  The call's ffi.RegenInfo;
        the run is finished when its live and remaining are both 0."""
        info = ffi.RegenInfo()
        check(self._lib, self._lib.vk_regen_step(self._h, batch._h, max_bounces, C.byref(info)))
        return info

    def regen_cull(self, batch, keep, scale=None):
        """PathBatch.cull()'s rule on a regenerating batch between two steps (vk_regen_cull): keep and scale in live order; a culled path
        is deposited as ffi.VK_PATHS_CULLED with its state as it stands."""
        n = int(batch.info().live)
        keep = np.ascontiguousarray(keep, np.uint8).reshape(-1)
        assert keep.shape[0] == n
        if scale is not None:
            scale = np.ascontiguousarray(scale, np.float32).reshape(-1)
            assert scale.shape[0] == n
        check(self._lib, self._lib.vk_regen_cull(self._h, batch._h, C.c_void_p(keep.ctypes.data if n else None),
                                                 C.c_void_p(scale.ctypes.data) if scale is not None and n else None))

    def render_regen(self, batch, cull=None, roulette=_KEEP):
        """The whole frame through `batch` by regenerating runs: one run over the whole frame per range of samples, the ranges chosen so
        that a run has fewer than 2^32 paths (one run, unless width * height * samples_per_pixel reaches that).  cull, where given, is
        called with the batch between two bounces while anything is live (PathBatch.read() and regen_cull() are its tools).  roulette,
        where given, is set on the batch first: (first_depth, q_min, q_max) or None (PathBatch.set_roulette); the rule runs on the
        device, so a run without a cull callback is still stepped in one call.  Returns resolve()."""
        if roulette is not Film._KEEP:
            batch.set_roulette(*(roulette or (None,)))
        p = self.params
        spp = p.samples_per_pixel
        ns = max(1, min(spp, (2 ** 32 - 1) // (p.width * p.height)))
        for s0 in range(0, spp, ns):
            self.regen_begin(batch, 0, 0, p.width, p.height, s0, min(ns, spp - s0))
            while True:
                info = self.regen_step(batch, 1 if cull is not None else 0xFFFFFFFF)
                if info.live == 0 and info.remaining == 0:
                    break
                if cull is not None and info.live:
                    cull(batch)
        return self.resolve()

    def enable_adaptive(self, abs_tol=None, rel_tol=0.0, min_samples=0, min_steps=2):
        """Error moments next to the sums (vk_adapt_enable), before the first emit or deposit since create / reset.  With abs_tol None
        moments only: no tile ever freezes.  Otherwise Progress.set_adaptive's rule runs behind every adapt_close()."""
        ap = None if abs_tol is None else ffi.AdaptiveParams(abs_tol, rel_tol, min_samples, min_steps)
        check(self._lib, self._lib.vk_adapt_enable(self._h, C.byref(ap) if ap is not None else None))

    def adapt_begin(self, batch, n_samples):
        """Put `batch` into its regenerating state for the tile window (vk_adapt_begin): the next n_samples samples of every pixel of
        every active tile; regen_step() and regen_cull() run it."""
        check(self._lib, self._lib.vk_adapt_begin(self._h, batch._h, n_samples))

    def adapt_close(self, n_samples):
        """Every pixel of every active tile has received its next n_samples samples (vk_adapt_close): fold them into the moments, judge
        the tiles, rebuild the list.  The ffi.AdaptInfo behind it."""
        info = ffi.AdaptInfo()
        check(self._lib, self._lib.vk_adapt_close(self._h, n_samples, C.byref(info)))
        return info

    def resolve_adaptive(self, out=None):
        """The frame of the last adapt_close(), every pixel the mean over its tile's own count (vk_adapt_resolve)"""
        p = self.params
        if out is None:
            out = np.zeros((p.height, p.width, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == p.width * p.height * 3
        check(self._lib, self._lib.vk_adapt_resolve(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def stderr(self):
        """Batch-means standard error of resolve_adaptive()'s frame (vk_adapt_stderr), float32 (height, width, 3), y = 0 the bottom row:
        the stderr3 image denoise() and Temporal.accumulate() take.  Two closes or more."""
        p = self.params
        out = np.zeros((p.height, p.width, 3), np.float32)
        check(self._lib, self._lib.vk_adapt_stderr(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def tile_samples(self):
        """(samples per tile as uint32 (tiles_y, tiles_x), tile row 0 at the bottom; vk_adaptive_info): Progress.tile_samples()' layout"""
        p = self.params
        out = np.zeros(((p.height + 7) // 8, (p.width + 7) // 8), np.uint32)
        inf = ffi.AdaptiveInfo()
        check(self._lib, self._lib.vk_adapt_tile_samples(self._h, out.ctypes.data_as(C.c_void_p), C.byref(inf)))
        return out, inf

    def render_adaptive(self, batch, window, cull=None):
        """Windows of `window` samples through tile runs — adapt_begin(), regen_step() to the run's end, adapt_close() — until the
        film's samples_per_pixel is reached or no tile is active.  cull as in render_regen().  Returns (resolve_adaptive(), the last
        close's ffi.AdaptInfo, None where no window was run); needs enable_adaptive()."""
        spp = self.params.samples_per_pixel
        tiles, inf = self.tile_samples()
        # (a frozen tile's count is at most samples_done, an active tile's is samples_done)
        done, active, info = int(tiles.max()), inf.tiles_active, None
        while active and done < spp:
            n = min(window, spp - done)
            self.adapt_begin(batch, n)
            while True:
                r = self.regen_step(batch, 1 if cull is not None else 0xFFFFFFFF)
                if r.live == 0 and r.remaining == 0:
                    break
                if cull is not None and r.live:
                    cull(batch)
            info = self.adapt_close(n)
            done, active = info.samples_done, info.tiles_active
        return self.resolve_adaptive(), info

    def debug_moments(self):
        """(the sums at the last close as int64, the error moments as float64), each (height, width, 3) y up: vk_debug_adapt_moments, a
        test hook in Progress.moments()' layout"""
        p = self.params
        run, m2 = np.zeros((p.height, p.width, 3), np.int64), np.zeros((p.height, p.width, 3), np.float64)
        check(self._lib, self._lib.vk_debug_adapt_moments(self._h, run.ctypes.data_as(C.c_void_p), m2.ctypes.data_as(C.c_void_p)))
        return run, m2

    def debug_set_tiles(self, tile_n, tile_k=None):
        """Impose a tile map (vk_debug_adapt_set_tiles, a test hook): tile_n (tiles_y, tiles_x), 0 = active; tile_k defaults to 2 where
        a tile is frozen"""
        p = self.params
        tile_n = np.ascontiguousarray(tile_n, np.uint32).reshape(-1)
        assert tile_n.size == ((p.height + 7) // 8) * ((p.width + 7) // 8)
        tile_k = np.where(tile_n != 0, 2, 0).astype(np.uint32) if tile_k is None else np.ascontiguousarray(tile_k, np.uint32).reshape(-1)
        assert tile_k.size == tile_n.size
        check(self._lib, self._lib.vk_debug_adapt_set_tiles(self._h, tile_n.ctypes.data_as(C.c_void_p), tile_k.ctypes.data_as(C.c_void_p)))

    def debug_sequence(self, n_samples, first, m):
        """(pixel, sample) uint32 arrays of paths first .. first + m of a tile run of n_samples over the current tile set, from the top-up
        kernel's index code on the device (vk_debug_adapt_sequence, a test hook)"""
        pixel, sample = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        check(self._lib, self._lib.vk_debug_adapt_sequence(self._h, n_samples, first, m, pixel.ctypes.data_as(C.c_void_p),
                                                           sample.ctypes.data_as(C.c_void_p)))
        return pixel, sample

    def regen_last_ms(self, batch):
        """(top-up, trace, shade, compaction with deposit) device milliseconds of the regenerating batch's last bounce
        (vk_debug_regen_last_ms, a test hook)"""
        ms = (C.c_double * 4)()
        check(self._lib, self._lib.vk_debug_regen_last_ms(batch._h, C.byref(ms)))
        return tuple(ms)

    def debug_sums(self):
        """The raw sums (vk_debug_film_sums, a test hook): int64 (height, width, 3) in 2^-26 units"""
        p = self.params
        out = np.zeros((p.height, p.width, 3), np.int64)
        check(self._lib, self._lib.vk_debug_film_sums(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def last_ms(self):
        """(emit, deposit, resolve) device milliseconds of the last call of each (vk_debug_film_last_ms, a test hook)"""
        ms = (C.c_double * 3)()
        check(self._lib, self._lib.vk_debug_film_last_ms(self._h, C.byref(ms)))
        return tuple(ms)

    def debug_deposit_form(self, form):
        """ffi.VK_DEBUG_FILM_DEPOSIT_PLAIN or _RUNS from the next deposit() on (vk_debug_film_deposit_form, a test hook)"""
        check(self._lib, self._lib.vk_debug_film_deposit_form(self._h, form))

    def close(self):
        if self._h:
            self._lib.vk_film_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Splat:
    """vk_splat handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): deposit() finished path
    batches, each sample spread over the pixels its filter reaches; resolve() divides the colour sums by the weight sums.  With
    ffi.VK_SPLAT_BOX at radius 0.5 the frame of a film's camera paths is render()'s, bit for bit."""

    def __init__(self, scene, width, height, spp, params):
        self._lib = scene._lib
        self._scene = scene
        self.width, self.height, self.spp = int(width), int(height), int(spp)
        self.params = ffi.SplatParams.from_buffer_copy(params)
        h = C.c_void_p()
        check(self._lib, self._lib.vk_splat_create(scene._h, width, height, spp, C.byref(self.params), C.byref(h)))
        self._h = h

    def deposit(self, batch, positions=None):
        """Splat the retired paths of `batch`, which has nothing live (vk_splat_deposit).  positions: None — each sample at its state's
        pixel, offset by the jitter its stream starts with (a film's camera paths) — or float32 (started, 2) frame coordinates."""
        ptr = None
        if positions is not None:
            positions = np.ascontiguousarray(positions, np.float32)
            assert positions.size == 2 * int(batch.info().started)
            ptr = positions.ctypes.data_as(C.c_void_p)
        check(self._lib, self._lib.vk_splat_deposit(self._h, batch._h, ptr))

    def resolve(self, out=None):
        """The filtered frame (vk_splat_resolve): float32 (height, width, 3), y = 0 the bottom row; a pixel whose weights sum to zero or
        less is black.  out: an array of that shape to write into."""
        if out is None:
            out = np.zeros((self.height, self.width, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == self.width * self.height * 3
        check(self._lib, self._lib.vk_splat_resolve(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def reset(self):
        """Zero the sums and the counters (vk_splat_reset)."""
        check(self._lib, self._lib.vk_splat_reset(self._h))

    def info(self):
        inf = ffi.SplatInfo()
        check(self._lib, self._lib.vk_splat_get_info(self._h, C.byref(inf)))
        return inf

    def render(self, film, batch, cull=None):
        """The whole frame of `film` through `batch`, filtered: Film.render()'s windows, each emitted, stepped to its end and deposited
        here instead of into the film.  Returns resolve()."""
        for win in film.windows(int(batch.info().capacity)):
            film.emit(batch, *win)
            while batch.step(1).live:
                if cull is not None:
                    cull(batch)
            self.deposit(batch)
        return self.resolve()

    def debug_sums(self):
        """The raw sums (vk_debug_splat_sums, a test hook): int64 (height, width, 4) in 2^-26 units — r, g, b, weight"""
        out = np.zeros((self.height, self.width, 4), np.int64)
        check(self._lib, self._lib.vk_debug_splat_sums(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_form(self, form):
        """ffi.VK_DEBUG_SPLAT_FORM_DEFAULT, _PLAIN or _TILED from the next deposit() on (vk_debug_splat_form, a test hook)"""
        check(self._lib, self._lib.vk_debug_splat_form(self._h, form))

    def last_ms(self):
        """(deposit, resolve) device milliseconds of the last call of each (vk_debug_splat_last_ms, a test hook)"""
        ms = (C.c_double * 2)()
        check(self._lib, self._lib.vk_debug_splat_last_ms(self._h, C.byref(ms)))
        return tuple(ms)

    def close(self):
        if self._h:
            self._lib.vk_splat_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Robust:
    """vk_robust handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): deposit() finished path
    batches into the buckets of their pixels; resolve() orders each pixel's buckets, trims and divides.  With ffi.VK_ROBUST_MEAN the
    frame of a film's camera paths is the film's, bit for bit."""

    def __init__(self, scene, width, height, spp, params):
        self._lib = scene._lib
        self._scene = scene
        self.width, self.height, self.spp = int(width), int(height), int(spp)
        self.params = ffi.RobustParams.from_buffer_copy(params)
        self.buckets = int(self.params.buckets)
        h = C.c_void_p()
        check(self._lib, self._lib.vk_robust_create(scene._h, width, height, spp, C.byref(self.params), C.byref(h)))
        self._h = h

    def deposit(self, batch):
        """Add the retired paths of `batch`, which has nothing live (vk_robust_deposit): sample s of a pixel goes to bucket s % buckets."""
        check(self._lib, self._lib.vk_robust_deposit(self._h, batch._h))

    def resolve(self, mode=None, trim=None, want_stderr=False, out=None):
        """The frame (vk_robust_resolve): float32 (height, width, 3), y = 0 the bottom row.  mode / trim: None — the accumulator's own —
        or another way to resolve the same sums.  want_stderr: return (image, stderr3), the standard error of the kept bucket means
        in the same layout.  out: an array of the image's shape to write into."""
        if out is None:
            out = np.zeros((self.height, self.width, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == self.width * self.height * 3
        how = None
        if mode is not None or trim is not None:
            how = C.byref(ffi.RobustParams(0, self.params.mode if mode is None else mode, self.params.trim if trim is None else trim, 0))
        se = np.zeros((self.height, self.width, 3), np.float32) if want_stderr else None
        check(self._lib, self._lib.vk_robust_resolve(self._h, how, out.ctypes.data_as(C.c_void_p),
                                                     se.ctypes.data_as(C.c_void_p) if want_stderr else None))
        return (out, se) if want_stderr else out

    def reset(self):
        """Zero the sums and the counters (vk_robust_reset)."""
        check(self._lib, self._lib.vk_robust_reset(self._h))

    def info(self):
        inf = ffi.RobustInfo()
        check(self._lib, self._lib.vk_robust_get_info(self._h, C.byref(inf)))
        return inf

    def render(self, film, batch, cull=None):
        """The whole frame of `film` through `batch`: Film.render()'s windows, each emitted, stepped to its end and deposited into the
        film and here.  Returns resolve()."""
        for win in film.windows(int(batch.info().capacity)):
            film.emit(batch, *win)
            while batch.step(1).live:
                if cull is not None:
                    cull(batch)
            film.deposit(batch)
            self.deposit(batch)
        return self.resolve()

    def debug_sums(self):
        """The raw state (vk_debug_robust_sums, a test hook): int64 (height, width, buckets, 4) — r, g, b in 2^-26 units, count"""
        out = np.zeros((self.height, self.width, self.buckets, 4), np.int64)
        check(self._lib, self._lib.vk_debug_robust_sums(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def last_ms(self):
        """(deposit, resolve) device milliseconds of the last call of each (vk_debug_robust_last_ms, a test hook)"""
        ms = (C.c_double * 2)()
        check(self._lib, self._lib.vk_debug_robust_last_ms(self._h, C.byref(ms)))
        return tuple(ms)

    def close(self):
        if self._h:
            self._lib.vk_robust_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


STANDARD_LAYERS = ("emission", "sky", "direct_diffuse", "direct_specular", "volume", "indirect", "rest")
_ANY_STATUS = (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED, ffi.VK_PATHS_CULLED)


class Tone:
    """vk_tone handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): the display transform of one
    width x height.  load() or load_device() a float frame (y = 0 the bottom row), meter() its exposure from a luminance histogram,
    encode() it through a tone curve and a transfer to uint8 (height, width, 3), row 0 the top, as VK_OUTPUT_RGB8.  With
    ffi.VK_TONE_CLAMP, ffi.VK_TONE_TRANSFER_REFERENCE and no metering the bytes are vk_to_color_device's."""

    def __init__(self, scene, width, height):
        self._lib = scene._lib
        self._scene = scene
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(self._lib, self._lib.vk_tone_create(scene._h, width, height, C.byref(h)))
        self._h = h

    def load(self, rgb):
        """The frame from host memory (vk_tone_load): float32, width * height * 3 values."""
        rgb = np.ascontiguousarray(rgb, np.float32)
        assert rgb.size == self.width * self.height * 3
        check(self._lib, self._lib.vk_tone_load(self._h, rgb.ctypes.data_as(C.c_void_p)))

    def load_device(self, d_rgb):
        """The frame from memory of the handle's device (vk_tone_load_device, enqueued on the null stream): a contiguous float32 tensor
        (an object with data_ptr()) of width * height * 3 values, or a device pointer."""
        if hasattr(d_rgb, "data_ptr"):
            assert d_rgb.is_contiguous() and d_rgb.numel() == self.width * self.height * 3 and d_rgb.element_size() == 4
            d_rgb = d_rgb.data_ptr()
        check(self._lib, self._lib.vk_tone_load_device(self._h, C.c_void_p(d_rgb)))

    @staticmethod
    def meter_params(**kw):
        """ffi.ToneMeterParams: the library's defaults (a loaded library is needed) with the given fields replaced"""
        mp = ffi.ToneMeterParams()
        lib = ffi.load_device_lib()
        check(lib, lib.vk_tone_default_meter_params(C.byref(mp)))
        for k, v in kw.items():
            setattr(mp, k, v)
        return mp

    @staticmethod
    def params(**kw):
        """ffi.ToneParams: the library's defaults (ACES, sRGB, the metered exposure) with the given fields replaced"""
        tp = ffi.ToneParams()
        lib = ffi.load_device_lib()
        check(lib, lib.vk_tone_default_params(C.byref(tp)))
        for k, v in kw.items():
            setattr(tp, k, v)
        return tp

    def meter(self, params=None, **kw):
        """Meter the loaded frame (vk_tone_meter): the histogram on the device, the exposure on the host.  params: an
        ffi.ToneMeterParams, or keywords over the defaults (key, low_fraction, high_fraction, blend, min_log2, max_log2).  Returns the
        ffi.ToneMeterInfo."""
        mp = params if params is not None else self.meter_params(**kw)
        info = ffi.ToneMeterInfo()
        check(self._lib, self._lib.vk_tone_meter(self._h, C.byref(mp), C.byref(info)))
        return info

    def encode(self, params=None, out=None, **kw):
        """The loaded frame as display codes (vk_tone_encode): uint8 (height, width, 3), row 0 the top.  params: an ffi.ToneParams, or
        keywords over the defaults (curve, transfer, flags, exposure, white, seed)."""
        tp = params if params is not None else self.params(**kw)
        if out is None:
            out = np.zeros((self.height, self.width, 3), np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size == self.width * self.height * 3
        check(self._lib, self._lib.vk_tone_encode(self._h, C.byref(tp), out.ctypes.data_as(C.c_void_p)))
        return out

    def encode_device(self, d_out, params=None, **kw):
        """The codes into memory of the handle's device (vk_tone_encode_device, enqueued on the null stream): a contiguous uint8 tensor of
        width * height * 3 values, or a 4-byte aligned device pointer.  Returns d_out."""
        tp = params if params is not None else self.params(**kw)
        ptr = d_out
        if hasattr(d_out, "data_ptr"):
            assert d_out.is_contiguous() and d_out.numel() == self.width * self.height * 3 and d_out.element_size() == 1
            ptr = d_out.data_ptr()
        check(self._lib, self._lib.vk_tone_encode_device(self._h, C.byref(tp), C.c_void_p(ptr)))
        return d_out

    def reset(self):
        """Forget the metered exposure and the frame (vk_tone_reset): the next meter is a first one."""
        check(self._lib, self._lib.vk_tone_reset(self._h))

    def info(self):
        inf = ffi.ToneInfo()
        check(self._lib, self._lib.vk_tone_get_info(self._h, C.byref(inf)))
        return inf

    def histogram(self):
        """The last meter's (bins (640,) uint32, counters (4,) uint64: binned, below, above, nonfinite) (vk_debug_tone_histogram, a test
        hook)"""
        bins, counters = np.zeros(640, np.uint32), np.zeros(4, np.uint64)
        check(self._lib, self._lib.vk_debug_tone_histogram(self._h, bins.ctypes.data_as(C.c_void_p), counters.ctypes.data_as(C.c_void_p)))
        return bins, counters

    def set_form(self, form):
        """The meter kernel's form, ffi.VK_TONE_FORM_LDS or _PLAIN (vk_debug_tone_set_form, a test hook)"""
        check(self._lib, self._lib.vk_debug_tone_set_form(self._h, form))

    def last_ms(self):
        """(meter, encode) device milliseconds of the last kernel of each (vk_debug_tone_last_ms, a test hook)"""
        ms = (C.c_double * 2)()
        check(self._lib, self._lib.vk_debug_tone_last_ms(self._h, C.byref(ms)))
        return tuple(ms)

    def close(self):
        if self._h:
            self._lib.vk_tone_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NonLocalMeans:
    """vk_nlm handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): non-local means over one
    width x height.  load() or load_device() a float frame, its per-channel standard error and, optionally, its albedo (y = 0 the
    bottom row, 3 floats a pixel); filter() or filter_device() it, as often as wanted and with other parameters, without a reload."""

    def __init__(self, scene, width, height):
        self._lib = scene._lib
        self._scene = scene
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(self._lib, self._lib.vk_nlm_create(scene._h, width, height, C.byref(h)))
        self._h = h

    def _host(self, img):
        img = np.ascontiguousarray(img, np.float32)
        assert img.size == self.width * self.height * 3
        return img

    def _device(self, t):
        if hasattr(t, "data_ptr"):
            assert t.is_contiguous() and t.numel() == self.width * self.height * 3 and t.element_size() == 4
            return t.data_ptr()
        return t

    def load(self, color, stderr3, albedo=None):
        """The frame from host memory (vk_nlm_load): float32 arrays of width * height * 3 values; albedo may be None."""
        color, stderr3 = self._host(color), self._host(stderr3)
        albedo = None if albedo is None else self._host(albedo)
        check(self._lib, self._lib.vk_nlm_load(self._h, color.ctypes.data_as(C.c_void_p), stderr3.ctypes.data_as(C.c_void_p),
                                               None if albedo is None else albedo.ctypes.data_as(C.c_void_p)))

    def load_device(self, d_color, d_stderr3, d_albedo=None):
        """The frame from memory of the handle's device (vk_nlm_load_device, enqueued on the null stream): contiguous float32 tensors
        (objects with data_ptr()) of width * height * 3 values, or device pointers; d_albedo may be None."""
        check(self._lib, self._lib.vk_nlm_load_device(self._h, C.c_void_p(self._device(d_color)), C.c_void_p(self._device(d_stderr3)),
                                                      None if d_albedo is None else C.c_void_p(self._device(d_albedo))))

    def params(self, **kw):
        """ffi.NlmParams: the defaults of the handle's library (vk_nlm_default_params) with the given fields replaced"""
        p = ffi.NlmParams()
        check(self._lib, self._lib.vk_nlm_default_params(C.byref(p)))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def filter(self, params=None, want_stderr=True, **kw):
        """The loaded frame filtered (vk_nlm_filter): (out, stderr3_out), float32 (height, width, 3) each; stderr3_out is None with
        want_stderr=False.  params: an ffi.NlmParams, or keywords over the defaults (search_radius, patch_radius, k, alpha,
        albedo_floor)."""
        p = params if params is not None else self.params(**kw)
        out = np.zeros((self.height, self.width, 3), np.float32)
        se = np.zeros((self.height, self.width, 3), np.float32) if want_stderr else None
        check(self._lib, self._lib.vk_nlm_filter(self._h, C.byref(p), out.ctypes.data_as(C.c_void_p),
                                                 None if se is None else se.ctypes.data_as(C.c_void_p)))
        return out, se

    def filter_device(self, d_out, d_stderr3_out=None, params=None, **kw):
        """The filtered frame into memory of the handle's device (vk_nlm_filter_device, enqueued on the null stream): contiguous float32
        tensors of width * height * 3 values, or device pointers; d_stderr3_out may be None.  Returns (d_out, d_stderr3_out)."""
        p = params if params is not None else self.params(**kw)
        check(self._lib, self._lib.vk_nlm_filter_device(self._h, C.byref(p), C.c_void_p(self._device(d_out)),
                                                        None if d_stderr3_out is None else C.c_void_p(self._device(d_stderr3_out))))
        return d_out, d_stderr3_out

    def reset(self):
        """Forget the frame (vk_nlm_reset): the next filter needs a load."""
        check(self._lib, self._lib.vk_nlm_reset(self._h))

    def info(self):
        inf = ffi.NlmInfo()
        check(self._lib, self._lib.vk_nlm_get_info(self._h, C.byref(inf)))
        return inf

    def set_form(self, form):
        """The filter kernel's form, ffi.VK_NLM_FORM_AUTO, _PLAIN or _TILED (vk_debug_nlm_set_form, a test hook)"""
        check(self._lib, self._lib.vk_debug_nlm_set_form(self._h, form))

    def last_ms(self):
        """(prepare, filter) device milliseconds of the last kernel of each (vk_debug_nlm_last_ms, a test hook)"""
        ms = (C.c_double * 2)()
        check(self._lib, self._lib.vk_debug_nlm_last_ms(self._h, C.byref(ms)))
        return tuple(ms)

    def close(self):
        if self._h:
            self._lib.vk_nlm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Psf:
    """vk_psf handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): the point-spread stage over
    one width x height for kernels up to kmax x kmax.  load() a (K, K, 3) kernel (Psf.star() makes one), then apply() a float frame from
    host memory or apply_device() one on the handle's device (y = 0 the bottom row, 3 floats a pixel); the kernel's transform is kept
    until the next load."""

    def __init__(self, scene, width, height, kmax):
        self._lib = scene._lib
        self._scene = scene
        self.width, self.height, self.kmax = int(width), int(height), int(kmax)
        h = C.c_void_p()
        check(self._lib, self._lib.vk_psf_create(scene._h, width, height, kmax, C.byref(h)))
        self._h = h

    @staticmethod
    def star(K, streaks=6, rotation=0.0, sharpness=8.0, chroma=0.0, lib=None):
        """A (K, K, 3) float32 star kernel (vk_psf_star): a compact core and `streaks` rays from `rotation` (radians); `chroma` sets
        the three channels' radial scales apart"""
        lib = lib if lib is not None else ffi.load_device_lib()
        out = np.zeros((K, K, 3), np.float32)
        check(lib, lib.vk_psf_star(K, streaks, rotation, sharpness, chroma, out.ctypes.data_as(C.c_void_p)))
        return out

    def _device(self, t, n=None):
        if hasattr(t, "data_ptr"):
            assert t.is_contiguous() and t.numel() == (n if n is not None else self.width * self.height * 3) and t.element_size() == 4
            return t.data_ptr()
        return t

    def params(self, **kw):
        """ffi.PsfParams: the defaults of the handle's library (vk_psf_default_params) with the given fields replaced"""
        p = ffi.PsfParams()
        check(self._lib, self._lib.vk_psf_default_params(C.byref(p)))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def load(self, kernel):
        """Loads a kernel (vk_psf_load): a float32 (K, K, 3) array, tap (kx, ky) at [ky, kx], y up; it is normalised per channel"""
        kernel = np.ascontiguousarray(kernel, np.float32)
        assert kernel.ndim == 3 and kernel.shape[0] == kernel.shape[1] and kernel.shape[2] == 3
        check(self._lib, self._lib.vk_psf_load(self._h, kernel.shape[0], kernel.ctypes.data_as(C.c_void_p)))

    def load_device(self, K, d_kernel):
        """Loads a kernel from memory of the handle's device (vk_psf_load_device): a contiguous float32 tensor of K * K * 3 values, or
        a device pointer"""
        check(self._lib, self._lib.vk_psf_load_device(self._h, K, C.c_void_p(self._device(d_kernel, K * K * 3))))

    def apply(self, rgb, params=None, **kw):
        """The frame with the point-spread function's glare (vk_psf_apply): float32 (height, width, 3) from a float32 array of width *
        height * 3 values.  params: an ffi.PsfParams, or keywords over the defaults (strength, threshold, form)."""
        p = params if params is not None else self.params(**kw)
        rgb = np.ascontiguousarray(rgb, np.float32)
        assert rgb.size == self.width * self.height * 3
        out = np.zeros((self.height, self.width, 3), np.float32)
        check(self._lib, self._lib.vk_psf_apply(self._h, C.byref(p), rgb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def apply_device(self, d_in, d_out=None, params=None, **kw):
        """The same in memory of the handle's device (vk_psf_apply_device, enqueued on the null stream): contiguous float32 tensors
        (objects with data_ptr()) of width * height * 3 values, or device pointers; d_out None = in place.  Returns d_out."""
        p = params if params is not None else self.params(**kw)
        if d_out is None:
            d_out = d_in
        check(self._lib, self._lib.vk_psf_apply_device(self._h, C.byref(p), C.c_void_p(self._device(d_in)), C.c_void_p(self._device(d_out))))
        return d_out

    def reset(self):
        check(self._lib, self._lib.vk_psf_reset(self._h))

    def last_pass_ms(self):
        """device milliseconds of the last apply's four passes in the LDS form (vk_psf_debug_last_pass_ms, a test hook)"""
        ms = (C.c_double * 4)()
        check(self._lib, self._lib.vk_psf_debug_last_pass_ms(self._h, C.byref(ms)))
        return list(ms)

    def info(self):
        inf = ffi.PsfInfo()
        check(self._lib, self._lib.vk_psf_get_info(self._h, C.byref(inf)))
        return inf

    def close(self):
        if self._h:
            self._lib.vk_psf_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Glare:
    """vk_glare handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): the glare stage over one
    width x height.  apply() a float frame from host memory or apply_device() one on the handle's device (y = 0 the bottom row, 3
    floats a pixel); nothing is kept between applies."""

    def __init__(self, scene, width, height):
        self._lib = scene._lib
        self._scene = scene
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(self._lib, self._lib.vk_glare_create(scene._h, width, height, C.byref(h)))
        self._h = h

    def _device(self, t):
        if hasattr(t, "data_ptr"):
            assert t.is_contiguous() and t.numel() == self.width * self.height * 3 and t.element_size() == 4
            return t.data_ptr()
        return t

    def params(self, **kw):
        """ffi.GlareParams: the defaults of the handle's library (vk_glare_default_params) with the given fields replaced"""
        p = ffi.GlareParams()
        check(self._lib, self._lib.vk_glare_default_params(C.byref(p)))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def apply(self, rgb, params=None, **kw):
        """The frame with glare (vk_glare_apply): float32 (height, width, 3) from a float32 array of width * height * 3 values.  params:
        an ffi.GlareParams, or keywords over the defaults (levels, strength, falloff, threshold)."""
        p = params if params is not None else self.params(**kw)
        rgb = np.ascontiguousarray(rgb, np.float32)
        assert rgb.size == self.width * self.height * 3
        out = np.zeros((self.height, self.width, 3), np.float32)
        check(self._lib, self._lib.vk_glare_apply(self._h, C.byref(p), rgb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def apply_device(self, d_in, d_out=None, params=None, **kw):
        """The frame with glare in memory of the handle's device (vk_glare_apply_device, enqueued on the null stream): contiguous
        float32 tensors (objects with data_ptr()) of width * height * 3 values, or device pointers; d_out None = in place.  Returns
        d_out."""
        p = params if params is not None else self.params(**kw)
        if d_out is None:
            d_out = d_in
        check(self._lib, self._lib.vk_glare_apply_device(self._h, C.byref(p), C.c_void_p(self._device(d_in)), C.c_void_p(self._device(d_out))))
        return d_out

    def info(self):
        inf = ffi.GlareInfo()
        check(self._lib, self._lib.vk_glare_get_info(self._h, C.byref(inf)))
        return inf

    def set_form(self, form):
        """The kernels' form, ffi.VK_GLARE_FORM_AUTO, _PLAIN or _FUSED (vk_debug_glare_set_form, a test hook)"""
        check(self._lib, self._lib.vk_debug_glare_set_form(self._h, form))

    def last_ms(self):
        """device milliseconds of the last apply's kernels (vk_debug_glare_last_ms, a test hook)"""
        ms = C.c_double()
        check(self._lib, self._lib.vk_debug_glare_last_ms(self._h, C.byref(ms)))
        return ms.value

    def close(self):
        if self._h:
            self._lib.vk_glare_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Upsample:
    """vk_upsample handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): guided upsampling from
    w x h to W x H.  load() the low frame from host memory or load_device() it from the handle's device, then apply() / apply_device()
    with the high guides (y = 0 the bottom row; colour, stderr3, albedo and normal 3 floats a pixel, depth 1).  The loaded frame stays
    until the next load or reset()."""

    def __init__(self, scene, w, h, W, H):
        self._lib = scene._lib
        self._scene = scene
        self.w, self.h, self.W, self.H = int(w), int(h), int(W), int(H)
        u = C.c_void_p()
        check(self._lib, self._lib.vk_upsample_create(scene._h, w, h, W, H, C.byref(u)))
        self._h = u

    def _host(self, a, n):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, np.float32)
        assert a.size == n, (a.size, n)
        return a, a.ctypes.data_as(C.c_void_p)

    def _device(self, t, n):
        if t is None:
            return None
        if hasattr(t, "data_ptr"):
            assert t.is_contiguous() and t.numel() == n and t.element_size() == 4
            return C.c_void_p(t.data_ptr())
        return C.c_void_p(t)

    def params(self, **kw):
        """ffi.UpsampleParams: the defaults of the handle's library (vk_upsample_default_params) with the given fields replaced"""
        p = ffi.UpsampleParams()
        check(self._lib, self._lib.vk_upsample_default_params(C.byref(p)))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def load(self, color, stderr3=None, albedo=None, normal=None, depth=None):
        """The low frame from host memory (vk_upsample_load): float32 arrays of w * h * 3 values (depth: w * h); all but color may be None"""
        n = self.w * self.h
        keep = [self._host(a, n * c) for a, c in ((color, 3), (stderr3, 3), (albedo, 3), (normal, 3), (depth, 1))]
        check(self._lib, self._lib.vk_upsample_load(self._h, *[k[1] for k in keep]))

    def load_device(self, color, stderr3=None, albedo=None, normal=None, depth=None):
        """The low frame from memory of the handle's device (vk_upsample_load_device, enqueued on the null stream): contiguous float32
        tensors (objects with data_ptr()) or device pointers"""
        n = self.w * self.h
        check(self._lib, self._lib.vk_upsample_load_device(self._h, *[self._device(t, n * c) for t, c in
                                                                      ((color, 3), (stderr3, 3), (albedo, 3), (normal, 3), (depth, 1))]))

    def apply(self, albedo=None, normal=None, depth=None, want_stderr=True, params=None, **kw):
        """The upsampled frame (vk_upsample_apply): (rgb, stderr3) as float32 (H, W, 3), stderr3 None when want_stderr is False.  albedo,
        normal, depth: the first-hit buffers at W x H, or None.  params: an ffi.UpsampleParams, or keywords over the defaults (sigma_z,
        normal_squarings, albedo_floor)."""
        p = params if params is not None else self.params(**kw)
        n = self.W * self.H
        keep = [self._host(a, n * c) for a, c in ((albedo, 3), (normal, 3), (depth, 1))]
        out = np.zeros((self.H, self.W, 3), np.float32)
        se = np.zeros((self.H, self.W, 3), np.float32) if want_stderr else None
        check(self._lib, self._lib.vk_upsample_apply(self._h, C.byref(p), *[k[1] for k in keep], out.ctypes.data_as(C.c_void_p),
                                                     se.ctypes.data_as(C.c_void_p) if want_stderr else None))
        return out, se

    def apply_device(self, d_out, d_stderr3=None, albedo=None, normal=None, depth=None, params=None, **kw):
        """The upsampled frame in memory of the handle's device (vk_upsample_apply_device, enqueued on the null stream): contiguous
        float32 tensors (objects with data_ptr()) or device pointers; d_stderr3 None = not wanted.  Returns (d_out, d_stderr3)."""
        p = params if params is not None else self.params(**kw)
        n = self.W * self.H
        check(self._lib, self._lib.vk_upsample_apply_device(self._h, C.byref(p), self._device(albedo, n * 3), self._device(normal, n * 3),
                                                            self._device(depth, n), self._device(d_out, n * 3), self._device(d_stderr3, n * 3)))
        return d_out, d_stderr3

    def reset(self):
        check(self._lib, self._lib.vk_upsample_reset(self._h))

    def info(self):
        inf = ffi.UpsampleInfo()
        check(self._lib, self._lib.vk_upsample_get_info(self._h, C.byref(inf)))
        return inf

    def set_form(self, form):
        """The filter kernel's form, ffi.VK_UPSAMPLE_FORM_AUTO, _PLAIN or _TILED (vk_debug_upsample_set_form, a test hook)"""
        check(self._lib, self._lib.vk_debug_upsample_set_form(self._h, form))

    def last_ms(self):
        """device milliseconds of the last apply's filter kernel (vk_debug_upsample_last_ms, a test hook)"""
        ms = C.c_double()
        check(self._lib, self._lib.vk_debug_upsample_last_ms(self._h, C.byref(ms)))
        return ms.value

    def close(self):
        if self._h:
            self._lib.vk_upsample_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lpe_rule(layer, sig_mask=0, sig_value=0, status=_ANY_STATUS, depth=(0, 0xFFFFFFFF), emitter=None):
    """One vk_lpe_rule: a result goes to `layer` when (sig & sig_mask) == sig_value, its status is one of `status`, depth[0] <=
    state.depth <= depth[1] and — with emitter, a material index — the last bounce hit that material."""
    mask = 0
    for s in status:
        mask |= 1 << s
    return ffi.LpeRule(sig_mask, sig_value, mask, depth[0], depth[1], 0xFFFFFFFF if emitter is None else emitter, layer, 0)


def lpe_events(*codes):
    """(sig_mask, sig_value) of a path whose first len(codes) bounces have these event codes (2 + ffi.VK_MAT_*, ffi.VK_LPE_*); a code of
    None leaves its bounce open and 0 asks for "no such bounce" — lpe_events(2, 5, 0) is camera, Lambertian, light and nothing after."""
    mask = value = 0
    for b, c in enumerate(codes):
        if c is not None:
            mask |= 0xF << (4 * b)
            value |= c << (4 * b)
    return mask, value


def standard_rules():
    """The rules of STANDARD_LAYERS, by a path's first bounces and its last: emission and sky seen by the camera; light (an emitter
    or the sky) reached right after one Lambertian bounce (direct diffuse) or one Metal or Dielectric bounce (direct specular or glass);
    every path whose first bounce scattered in a medium (volume); whatever else ended on an emitter or the sky (indirect); the rest —
    paths that carry nothing: ended by the depth or an absorbing Metal, culled, bad."""
    L = {name: i for i, name in enumerate(STANDARD_LAYERS)}
    lamb, metal, glass, iso = (2 + m for m in (ffi.VK_MAT_LAMBERTIAN, ffi.VK_MAT_METAL, ffi.VK_MAT_DIELECTRIC, ffi.VK_MAT_ISOTROPIC))
    ended, missed = (ffi.VK_SHADE_ENDED,), (ffi.VK_SHADE_MISS,)
    rules = [lpe_rule(L["emission"], *lpe_events(ffi.VK_LPE_EMIT), status=ended), lpe_rule(L["sky"], *lpe_events(ffi.VK_LPE_SKY), status=missed)]
    for first, layer in ((lamb, "direct_diffuse"), (metal, "direct_specular"), (glass, "direct_specular")):
        rules.append(lpe_rule(L[layer], *lpe_events(first, ffi.VK_LPE_EMIT, 0), status=ended))
        rules.append(lpe_rule(L[layer], *lpe_events(first, ffi.VK_LPE_SKY, 0), status=missed))
    rules.append(lpe_rule(L["volume"], *lpe_events(iso)))
    rules.append(lpe_rule(L["indirect"], 0xF0000000, ffi.VK_LPE_EMIT << 28, status=ended))
    rules.append(lpe_rule(L["indirect"], 0xF0000000, ffi.VK_LPE_SKY << 28, status=missed))
    return rules


class LightPathLayers:
    """vk_lpe handle over a DeviceScene (close it, or leave the `with` block, before the scene is closed): step() a path batch as
    PathBatch.step() does while the tracker records every bounce's event per path, deposit() the finished batch into the layers its
    results' classes name, resolve() a layer.  All layers together are the film's frame, bit for bit."""

    def __init__(self, scene, width, height, spp, capacity, rules, n_layers, rest_layer):
        self._lib = scene._lib
        self._scene = scene
        self.width, self.height, self.spp, self.capacity = int(width), int(height), int(spp), int(capacity)
        self.rules = [ffi.LpeRule.from_buffer_copy(r) for r in rules]
        self.n_layers, self.rest_layer = int(n_layers), int(rest_layer)
        arr = (ffi.LpeRule * max(1, len(self.rules)))(*self.rules)
        lp = ffi.LpeParams(self.n_layers, self.rest_layer, len(self.rules), 0, arr if self.rules else None)
        h = C.c_void_p()
        check(self._lib, self._lib.vk_lpe_create(scene._h, width, height, spp, capacity, C.byref(lp), C.byref(h)))
        self._h = h

    def step(self, batch, max_bounces=1):
        """PathBatch.step() with the tags kept (vk_lpe_step): the call's ffi.PathsStepInfo, six launches a bounce.  The first step of a
        begun or emitted batch binds the tracker to it."""
        info = ffi.PathsStepInfo()
        check(self._lib, self._lib.vk_lpe_step(self._h, batch._h, max_bounces, C.byref(info)))
        return info

    def tags(self, batch):
        """(sig, term) uint32 arrays per started id of the bound batch (vk_lpe_tags)"""
        n = int(batch.info().started)
        sig, term = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data if n else None)
        check(self._lib, self._lib.vk_lpe_tags(self._h, batch._h, ptr(sig), ptr(term)))
        return sig, term

    def deposit(self, batch):
        """Add the retired paths of the bound `batch`, which has nothing live, each to the layer of its class (vk_lpe_deposit)."""
        check(self._lib, self._lib.vk_lpe_deposit(self._h, batch._h))

    def resolve(self, layer=ffi.VK_LPE_ALL, n=None, want_share=False, out=None):
        """A layer's image as its sums over n samples per pixel (vk_lpe_resolve; default: the tracker's spp): float32 (height, width, 3),
        y = 0 the bottom row; ffi.VK_LPE_ALL: every layer together, the film's frame.  want_share: return (image, share), share (height,
        width) the layer's part of the pixel's samples."""
        if out is None:
            out = np.zeros((self.height, self.width, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == self.width * self.height * 3
        share = np.zeros((self.height, self.width), np.float32) if want_share else None
        check(self._lib, self._lib.vk_lpe_resolve(self._h, layer, self.spp if n is None else n, out.ctypes.data_as(C.c_void_p),
                                                  share.ctypes.data_as(C.c_void_p) if want_share else None))
        return (out, share) if want_share else out

    def reset(self):
        """Zero the sums and the counters (vk_lpe_reset)."""
        check(self._lib, self._lib.vk_lpe_reset(self._h))

    def info(self):
        inf = ffi.LpeInfo()
        check(self._lib, self._lib.vk_lpe_get_info(self._h, C.byref(inf)))
        return inf

    def render(self, film, batch, cull=None):
        """The whole frame of `film` through `batch`: Film.render()'s windows, each emitted, stepped to its end here and deposited into
        the film and into the layers.  Returns the list of every layer's image."""
        for win in film.windows(min(int(batch.info().capacity), self.capacity)):
            film.emit(batch, *win)
            while self.step(batch, 1).live:
                if cull is not None:
                    cull(batch)
            film.deposit(batch)
            self.deposit(batch)
        return [self.resolve(layer) for layer in range(self.n_layers)]

    def debug_sums(self):
        """The raw state (vk_debug_lpe_sums, a test hook): int64 (height, width, n_layers, 4) — r, g, b in 2^-26 units, count"""
        out = np.zeros((self.height, self.width, self.n_layers, 4), np.int64)
        check(self._lib, self._lib.vk_debug_lpe_sums(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_set_tags(self, batch, sig, term):
        """Upload the tags of the batch's started ids and bind the tracker to it, every bounce counted as recorded
        (vk_debug_lpe_set_tags, a test hook)"""
        sig, term = np.ascontiguousarray(sig, np.uint32).reshape(-1), np.ascontiguousarray(term, np.uint32).reshape(-1)
        assert len(sig) == len(term) == int(batch.info().started)
        ptr = lambda a: C.c_void_p(a.ctypes.data if len(a) else None)
        check(self._lib, self._lib.vk_debug_lpe_set_tags(self._h, batch._h, ptr(sig), ptr(term)))

    def last_ms(self):
        """(record, deposit, resolve) device milliseconds of the last launch of each (vk_debug_lpe_last_ms, a test hook)"""
        ms = (C.c_double * 3)()
        check(self._lib, self._lib.vk_debug_lpe_last_ms(self._h, C.byref(ms)))
        return tuple(ms)

    def close(self):
        if self._h:
            self._lib.vk_lpe_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
