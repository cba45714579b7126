"""The oracle bridge for radiance queries (vk_trace_radiance).  TESTS ONLY; shared by the CPU and the GPU test.

vk::Rng is counter-based, so a sample of vk_render is "the camera's draws, then ray_color on the same stream".  The bridge takes each
sample's primary ray from the oracle (first_hits), replays the camera's draws to find how far its stream had advanced when ray_color
began, and hands the query that ray (tmax = +inf) with the key (seed, pixel, sample, ctr): the query's sample must then be the
oracle's sample (render_samples) — same final counter, same finite mask, radiance equal to re-association error.

The replay restates main.rs:186-190 / Camera::get_ray: two jitter draws; pairs of gen_range(-1, 1) until a*a + b*b < 1 in f32
(random_in_unit_disk, util.rs:41-50, drawn whatever the lens radius); gen_range(time0, time1) with its redraw loop.  It checks itself:
the time it computes equals first_hits' time bit for bit, for every sample."""
import numpy as np

from vecchio_amd.scene import KEY_DTYPE, make_rays

f32 = np.float32
N_DRAWS = 96          # draws looked at per sample (the disk loop accepts 79 % of its pairs)


def camera_ctr_and_time(oracle, seed, pixel, s, time0, time1):
    """(draws the camera took of the stream of (seed, pixel, s), the ray's time)"""
    # gen_range(-1, 1) takes exactly one draw each time (its redraw test cannot fire) and v01 = (r + 1) / 2 exactly
    r = oracle.draws(seed, pixel, s, 1, N_DRAWS, -1.0, 1.0)
    at = 2                                    # u and v jitter
    while True:
        a, b = r[at], r[at + 1]
        at += 2
        if f32(f32(f32(a * a) + f32(b * b)) + f32(0.0)) < f32(1.0):
            break
    lo, hi = f32(time0), f32(time1)
    scale = f32(hi - lo)
    while True:
        v01 = f32(f32(r[at] + f32(1.0)) * f32(0.5))
        at += 1
        res = f32(f32(v01 * scale) + lo)
        if res < hi:
            return at, res


def bridge(oracle, desc, cam, p):
    """(rays RAY_DTYPE, keys KEY_DTYPE, ref (n, 4) float32): one ray and key per (pixel, sample) of the frame in render_samples' order
    (pixel * spp + s, pixel = y * width + x), and the oracle's per-sample result"""
    spp = p.samples_per_pixel
    fh = oracle.first_hits(desc, cam, p, 0, spp).reshape(-1)
    n = p.width * p.height * spp
    assert len(fh) == n
    keys = np.zeros(n, KEY_DTYPE)
    keys["seed"] = p.seed
    for i in range(n):
        pixel, s = divmod(i, spp)
        ctr, t = camera_ctr_and_time(oracle, p.seed, pixel, s, cam.time0, cam.time1)
        # the replay's own check: no sample excepted
        assert f32(t).view(np.uint32) == fh["time"][i].view(np.uint32), (pixel, s, t, fh["time"][i])
        keys["pixel"][i], keys["sample"][i], keys["ctr"][i] = pixel, s, ctr
    rays = make_rays(fh["origin"], fh["direction"], fh["time"], np.inf)
    _, ref = oracle.render_samples(desc, cam, p)
    return rays, keys, ref


def radiance_kwargs(p):
    """the radiance parameters that go with render parameters p (samples_per_ray = 1: one ray per sample)"""
    return dict(seed=p.seed, first_index=0, samples_per_ray=1, first_sample=0, max_depth=p.max_depth, integrator=p.integrator,
                background=p.background, background_color=tuple(p.background_color))


def compare(ref, got):
    """what tests/test_emu_parity.compare demands of the emulator's samples: equal final counters, equal finite masks, relative radiance
    error < 2e-5 with its 1e-3 floor"""
    ref, got = ref.reshape(-1, 4), got.reshape(-1, 4)
    d_o, d_e = ref[:, 3].view(np.uint32), got[:, 3].view(np.uint32)
    assert np.array_equal(d_o, d_e), f"{int((d_o != d_e).sum())} of {len(d_o)} samples took a different path (final counters differ)"
    fo, fe = np.isfinite(ref[:, :3]).all(1), np.isfinite(got[:, :3]).all(1)
    assert np.array_equal(fo, fe), "finite filter (main.rs:192-194) would drop different samples"
    a, b = ref[fo, :3], got[fo, :3]
    rel = np.abs(a - b) / (np.abs(a) + 1e-3)
    assert rel.size == 0 or rel.max() < 2e-5, f"per-sample radiance differs by {rel.max()}"
    return float(rel.max()) if rel.size else 0.0
