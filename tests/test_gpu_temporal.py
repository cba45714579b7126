"""-m gpu: temporal accumulation (vk_temporal_*) on the MI355X, bit for bit against the numpy restatement of its definition
(tests/temporal_ref.py) on synthetic and rendered frame sequences; every call shape; reset; non-interference with vk_render, vk_denoise and
progress handles; invalid calls; the CLI; and what the history buys on an orbiting and on a fixed camera."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as R
from vecchio_amd import DeviceScene, HostScene, build, ffi

pytestmark = pytest.mark.gpu

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    bad = bits(got) != bits(want)
    if bad.ndim == 3:
        bad = bad.any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:3].tolist()}"


_ds = {}


def scene(name="cornell_box", **kw):
    key = (name, tuple(sorted(kw.items(), key=str)))
    if key not in _ds:
        hs = HostScene(name, 1)
        _ds[key] = (hs, hs.next_camera(), DeviceScene(hs.desc, **{k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}))
    return _ds[key]


def run_frame(t, cam, g, stderr=True, albedo=True, want_history=True):
    return t.accumulate(cam if isinstance(cam, ffi.Camera) else R.to_ffi(cam), g["color"], g["normal"], g["depth"],
                        stderr=g["stderr3"] if stderr else None, albedo=g["albedo"] if albedo else None, want_history=want_history)


def ref_frame(acc, cam, g, stderr=True, albedo=True):
    return acc.accumulate(cam, g["color"], g["stderr3"] if stderr else None, g["albedo"] if albedo else None, g["normal"], g["depth"])


def check_sequence(ds, seq, w, h, what, stderr=True, albedo=True, **over):
    """the frames of seq through a fresh handle and a fresh reference: every output of every frame bit for bit, and the counter"""
    kw = dict(R.DEFAULTS)
    kw.update(over)
    acc = R.Accumulator(w, h, **kw)
    shares = []
    with ds.temporal(w, h, **over) as t:
        for i, (cam, g) in enumerate(seq):
            c, s, n, st = run_frame(t, cam, g, stderr, albedo)
            rc, rs, rn = ref_frame(acc, cam, g, stderr, albedo)
            same(c, rc, f"{what}: colour of frame {i}")
            same(n, rn, f"{what}: history length of frame {i}")
            if stderr:
                same(s, rs, f"{what}: standard error of frame {i}")
            else:
                assert s is None
            inf = t.info()
            assert (inf.frames, inf.width, inf.height) == (i + 1, w, h)
            assert inf.pixels_with_history == int(acc.took.sum()), (what, i)
            assert st.samples == w * h and st.kernel_launches == 1 and st.kernel_ms > 0
            shares.append(inf.pixels_with_history / (w * h))
    return shares


@pytest.mark.parametrize("width,height", [(2, 2), (3, 200), (37, 29), (256, 144)])
def test_synthetic_sequences_bit_for_bit(width, height, device):
    hs, cam, ds = scene()
    for frames in range(1, 7):
        seq = R.synthetic(width, height, seed=width + frames, frames=frames)
        shares = check_sequence(ds, seq, width, height, f"{width}x{height}, {frames} frames")
        assert shares[0] == 0
        if frames > 1 and width >= 37:
            assert shares[-1] > 0.5                                     # the history was found
    g = R.synthetic(width, height, seed=3, frames=2)[1][1]
    assert width * height < 12 or not (np.isfinite(g["color"]).all() and np.isfinite(g["stderr3"]).all())
    if width * height > 10000:
        assert np.isinf(g["depth"]).any() and ((g["normal"] == 0).all(-1) & np.isfinite(g["depth"])).any()   # misses; hits without a normal
    seq = R.synthetic(width, height, seed=9, frames=4, step_deg=2.0)
    check_sequence(ds, seq, width, height, "other parameters", max_history=3, depth_tol=0.004, normal_cos_min=0.995, albedo_floor=0.25)
    check_sequence(ds, seq, width, height, "max_history 1", max_history=1)


def test_every_combination_of_the_optional_inputs_and_outputs(device):
    hs, cam, ds = scene()
    w, h = 37, 29
    seq = R.synthetic(w, h, seed=2, frames=3)
    outs = set()
    for stderr, albedo in itertools.product((False, True), repeat=2):
        check_sequence(ds, seq, w, h, f"stderr {stderr} albedo {albedo}", stderr=stderr, albedo=albedo)
        for want_se, want_n in itertools.product((False, True), repeat=2):
            if want_se and not stderr:
                continue
            acc = R.Accumulator(w, h)
            with ds.temporal(w, h) as t:
                for cam_i, g in seq:
                    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
                    c, s, n = np.zeros((h, w, 3), f32), np.full((h, w, 3), 7.0, f32), np.full((h, w), 7.0, f32)
                    rc = ds._lib.vk_temporal_accumulate(t._h, C.byref(R.to_ffi(cam_i)), ptr(g["color"]), ptr(g["stderr3"] if stderr else None),
                                                        ptr(g["albedo"] if albedo else None), ptr(g["normal"]), ptr(g["depth"]), ptr(c),
                                                        ptr(s if want_se else None), ptr(n if want_n else None), None)
                    assert rc == ffi.VK_OK
                    rcol, rs, rn = ref_frame(acc, cam_i, g, stderr, albedo)
                    same(c, rcol, "colour")
                    same(s, rs if want_se else np.full((h, w, 3), 7.0, f32), "standard error (or untouched)")
                    same(n, rn if want_n else np.full((h, w), 7.0, f32), "history (or untouched)")
            outs.add((stderr, albedo, c.tobytes()))
    assert len({o[2] for o in outs}) >= 2                               # demodulation does something


def test_a_camera_that_turns_away_finds_no_history(device):
    hs, cam, ds = scene()
    w, h = 64, 36
    seq = R.synthetic(w, h, seed=4, frames=3, turn_away=True)
    shares = check_sequence(ds, seq, w, h, "turned away")
    assert shares[1] > 0.5 and shares[2] == 0


def rendered(hs, ds, cam, w, h, spp, seed, windows=2, depth=50):
    p = hs.params(w, spp, depth, seed=seed, height=h)
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(windows):
            img, _ = pr.step(spp // windows)
        se = pr.stderr()
    aov, _ = ds.render_aov(cam, p)
    return dict(color=img.copy(), stderr3=se, albedo=aov["albedo"], normal=aov["normal"], depth=aov["depth"])


def rendered_sequence(name, w, h, frames, spp, fixed=False, seed0=5):
    hs = HostScene(name, 1)
    ds = DeviceScene(hs.desc)
    first = hs.next_camera()
    cams = [first] + [first if fixed else hs.next_camera() for _ in range(frames - 1)]
    return hs, ds, [(cams[i], rendered(hs, ds, cams[i], w, h, spp, seed0 + i)) for i in range(frames)]


@pytest.mark.parametrize("name,width,height,fixed", [("random_spheres_demo", 128, 72, False), ("cornell_box", 64, 64, True)])
def test_rendered_sequences_bit_for_bit(name, width, height, fixed, device):
    hs, ds, seq = rendered_sequence(name, width, height, 4, 8, fixed)
    try:
        if not fixed:
            assert bytes(seq[0][0]) != bytes(seq[1][0])                 # the RotatingCamera moved
        shares = check_sequence(ds, seq, width, height, name)
        assert shares[0] == 0 and min(shares[1:]) > 0.8, shares
    finally:
        ds.close()
        hs.close()


def test_device_call_multi_device_scene_and_reset(device):
    import torch
    hs, cam, ds = scene()
    w, h = 256, 144
    seq = R.synthetic(w, h, seed=1, frames=3)
    host = []
    with ds.temporal(w, h) as t:
        for cam_i, g in seq:
            host.append(run_frame(t, cam_i, g)[:3])
        # reset: the next frame is a first frame, and the sequence repeats bit for bit
        t.reset()
        assert t.info().frames == 0 and t.info().pixels_with_history == 0
        for (cam_i, g), want in zip(seq, host):
            got = run_frame(t, cam_i, g)[:3]
            for a, b in zip(got, want):
                same(a, b, "after reset")
    assert (host[0][2] <= 1).all() and (host[2][2] > 2).any()
    # the device call
    with ds.temporal(w, h) as t:
        for (cam_i, g), want in zip(seq, host):
            dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in g.items()}
            oc = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
            os_, on = torch.full_like(oc, 7.0), torch.full((h, w), 7.0, dtype=torch.float32, device="cuda:0")
            t.accumulate_device(R.to_ffi(cam_i), dev["color"].data_ptr(), dev["normal"].data_ptr(), dev["depth"].data_ptr(), oc.data_ptr(),
                                d_stderr=dev["stderr3"].data_ptr(), d_albedo=dev["albedo"].data_ptr(), d_out_stderr=os_.data_ptr(),
                                d_out_history=on.data_ptr())
            torch.cuda.synchronize()
            for a, b in zip((oc, os_, on), want):
                same(a.cpu().numpy(), b, "device call")
        assert t.info().pixels_with_history == int((host[2][2] > 1).sum())
    # a multi-device scene: on devices[0]
    _, _, multi = scene("cornell_box", devices=(0, 0))
    with multi.temporal(w, h) as t:
        for (cam_i, g), want in zip(seq, host):
            for a, b in zip(run_frame(t, cam_i, g)[:3], want):
                same(a, b, "multi-device scene")


def test_render_denoise_and_progress_are_not_disturbed(device):
    import denoise_ref
    hs, cam, ds = scene("random_spheres_iow")
    p = hs.params(64, 16, 50, seed=4, height=48)
    seq = R.synthetic(64, 48, seed=9, frames=3)
    dn_in = denoise_ref.synthetic(64, 48, seed=9)
    dn = lambda: ds.denoise(dn_in["color"], dn_in["stderr3"], dn_in["albedo"], dn_in["normal"], dn_in["depth"])[0]
    launches = lambda: [bytes(x) for x in ffi.last_launches(ds._lib, ds._h)]
    acc = R.Accumulator(64, 48)
    with ds.temporal(64, 48) as t:
        a, sa = ds.render(cam, p)
        clean = dn()
        la, ra, ms = launches(), ds.last_requeued_samples(), ds.last_kernel_ms()
        same(run_frame(t, *seq[0])[0], ref_frame(acc, *seq[0])[0], "frame 0")
        assert launches() == la and ds.last_requeued_samples() == ra and ds.last_kernel_ms() == ms
        b, sb = ds.render(cam, p)
        same(b, a, "vk_render after an accumulate call")
        assert launches() == la and ds.last_requeued_samples() == ra and sb.clamped_samples == sa.clamped_samples
        same(dn(), clean, "vk_denoise after an accumulate call")
        with ds.progress(cam, p) as pr:                # a progress handle interrupted by an accumulate call
            pr.step(6)
            same(run_frame(t, *seq[1])[0], ref_frame(acc, *seq[1])[0], "frame 1, between a render, a denoise call and a progress step")
            img, _ = pr.step(10)
        same(img, a, "progress handle around an accumulate call")
        same(run_frame(t, *seq[2])[0], ref_frame(acc, *seq[2])[0], "frame 2")


def test_invalid_calls_leave_the_outputs_and_the_history_untouched(device):
    hs, cam, ds = scene()
    lib = ds._lib
    w, h = 16, 16
    seq = R.synthetic(w, h, seed=4, frames=3, invalid=False)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    hnd = C.c_void_p()
    for over in (dict(width=1), dict(max_history=0), dict(max_history=65536), dict(depth_tol=0.0), dict(depth_tol=float("nan")),
                 dict(normal_cos_min=2.0), dict(albedo_floor=-1.0), dict(flags=1)):
        tp = ffi.TemporalParams()
        lib.vk_temporal_default_params(w, h, C.byref(tp))
        for k, v in over.items():
            setattr(tp, k, v)
        assert lib.vk_temporal_create(ds._h, C.byref(tp), C.byref(hnd)) == ffi.VK_ERR_BAD_ARG and not hnd.value, over
    acc = R.Accumulator(w, h)
    with ds.temporal(w, h) as t:
        (c0, g0), (c1, g1), (c2, g2) = seq
        same(run_frame(t, c0, g0)[0], ref_frame(acc, c0, g0)[0], "frame 0")
        cam1 = R.to_ffi(c1)
        sent3, sent1 = np.full((h, w, 3), 7.0, f32), np.full((h, w), 7.0, f32)
        oc, os_, on = sent3.copy(), sent3.copy(), sent1.copy()
        good = [ptr(g1["color"]), ptr(g1["stderr3"]), ptr(g1["albedo"]), ptr(g1["normal"]), ptr(g1["depth"]), ptr(oc), ptr(os_), ptr(on)]
        call = lambda args, c=cam1: lib.vk_temporal_accumulate(t._h, C.byref(c) if c is not None else None, *args, None)
        for k in (0, 3, 4, 5):                        # a required pointer missing
            args = list(good)
            args[k] = None
            assert call(args) == ffi.VK_ERR_BAD_ARG, k
        assert call(good, None) == ffi.VK_ERR_BAD_ARG                   # no camera
        args = list(good)
        args[1] = None                                                  # out_stderr3 without stderr3
        assert call(args) == ffi.VK_ERR_BAD_ARG and b"stderr3" in lib.vk_last_error()
        alias = g1["color"].copy()
        for k in (0, 1, 2, 3):                        # out_color aliasing an input, whichever
            args = [ptr(g1["color"]), ptr(g1["stderr3"]), ptr(g1["albedo"]), ptr(g1["normal"]), ptr(g1["depth"]), ptr(alias), ptr(os_), ptr(on)]
            args[k] = ptr(alias)
            assert call(args) == ffi.VK_ERR_BAD_ARG, k
        args = list(good)
        args[6] = ptr(oc)                                               # two outputs on one buffer
        assert call(args) == ffi.VK_ERR_BAD_ARG
        args = list(good)
        args[7] = C.c_void_p(g1["depth"].ctypes.data + 16)              # out_history inside depth
        assert call(args) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_temporal_accumulate_device(t._h, C.byref(cam1), None, None, None, None, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
        np.testing.assert_array_equal(alias, g1["color"])
        for a, s in ((oc, sent3), (os_, sent3), (on, sent1)):
            np.testing.assert_array_equal(a, s)
        assert t.info().frames == 1
        # the next valid frames are what they would have been
        for cam_i, g in ((c1, g1), (c2, g2)):
            got, want = run_frame(t, cam_i, g), ref_frame(acc, cam_i, g)
            for a, b in zip(got[:3], want):
                same(a, b, "after the refused calls")


def _read_pfm(path):
    raw = path.read_bytes()
    head, rest = raw.split(b"\n", 3)[:3], raw.split(b"\n", 3)[3]
    (w, h) = map(int, head[1].split())
    assert head[0] == b"PF" and float(head[2]) == -1.0 and len(rest) == w * h * 12
    return np.frombuffer(rest, dtype="<f4").reshape(h, w, 3)


def test_cli_accumulates_the_frames(device, tmp_path):
    cli = build.build_cli()
    a, b, c = tmp_path / "ten", tmp_path / "off", tmp_path / "on"
    a.mkdir(), b.mkdir(), c.mkdir()
    env = dict(os.environ, VECCHIO_ASSETS=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assets"))
    base = [cli, "random_spheres_demo", "64", "8", "10", "3", "1", "2", "8", "1"]
    subprocess.run(base, cwd=a, check=True, timeout=600, capture_output=True, env=env)
    subprocess.run(base + ["0"], cwd=b, check=True, timeout=600, capture_output=True, env=env)
    subprocess.run(base + ["1"], cwd=c, check=True, timeout=600, capture_output=True, env=env)
    names = sorted(f.name for f in a.iterdir())
    assert len(names) == 3 * (2 + 4 + 2 + 2) and "output_0002_denoised.pfm" in names
    assert sorted(f.name for f in b.iterdir()) == names
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n         # temporal = 0: what it was
    extra = [f"output_{i:04d}_temporal.{ext}" for i in range(3) for ext in ("ppm", "pfm")]
    assert sorted(f.name for f in c.iterdir()) == sorted(names + extra)
    assert (a / "output_0000.pfm").read_bytes() == (c / "output_0000.pfm").read_bytes()        # frame 0: seed + 1, as ever
    assert (a / "output_0001.pfm").read_bytes() != (c / "output_0001.pfm").read_bytes()        # frame 1: another seed
    for argv in (base[:7] + ["1", "8", "0", "1"], base[:8] + ["0", "0", "1"]):                  # refused without stderr / AOVs
        r = subprocess.run(argv, cwd=tmp_path, timeout=300, capture_output=True)
        assert r.returncode != 0 and b"temporal" in r.stderr
    # the same pipeline from Python
    hs = HostScene("random_spheres_demo", 1)
    ds = DeviceScene(hs.desc)
    try:
        h = hs.params(64, 8, 10).height
        with ds.temporal(64, h) as t:
            for i in range(3):
                cam = hs.next_camera()
                g = rendered(hs, ds, cam, 64, h, 8, 2 + i, windows=2, depth=10)
                same(_read_pfm(c / f"output_{i:04d}.pfm"), g["color"], f"the CLI's frame {i}")
                color, se, _, _ = run_frame(t, cam, g, want_history=False)
        same(_read_pfm(c / "output_0002_temporal.pfm"), color, "CLI, accumulated frame 2")
        clean, _ = ds.denoise(color, se, g["albedo"], g["normal"], g["depth"])
        same(_read_pfm(c / "output_0002_denoised.pfm"), clean, "CLI, accumulated and denoised frame 2")
    finally:
        ds.close()
        hs.close()


def rel_mse(img, truth):
    return float(np.mean((img.astype(np.float64) - truth) ** 2 / (truth.astype(np.float64) ** 2 + 1e-2)))


# tools/temporal_report.py --part orbit measured, on random_spheres_demo 256x144 under its RotatingCamera (8 frames at 8 spp in 2 windows,
# AOVs at 8 spp, seed 5 + frame, defaults, against 8192 spp of frame 8's camera with seed 77), the ratio relMSE(frame 8 accumulated and
# denoised) / relMSE(frame 8 denoised alone) as R_ORBIT_MEASURED; the pipeline must keep at least half of that improvement —
# ratio <= 1 - (1 - r) / 2 — the margin covering the change of seed.  The run it came from: R_MEASURED_RUN and DESIGN.md.
R_ORBIT_MEASURED = 0.6497       # relMSE 0.062590 (denoised alone) -> 0.040666 (accumulated, then denoised); the noisy frame 0.094643
# --part fixed: cornell_box 128x128 under its fixed camera, 8 frames at 4 spp accumulated against ONE 32-spp vk_render frame, over 5 seed
# sets.  Eight independent 4-spp means are a 32-spp estimator, so the ratio is expected near 1; the bound is mean + 3 x (max - min).
R_FIXED_MEASURED = (0.7223, 0.8733, 1.0523, 0.8996, 1.8839)      # mean 1.0863, max - min 1.1616 (a few outlying pixels: DESIGN.md)
# That spread makes the bound above loose (4.57), so the same rule is also applied to a figure that outlying pixels do not move: the
# median over the pixels of the per-pixel relative squared error (its mean over the three components), the same five seed sets.
R_FIXED_MEDIAN_MEASURED = (1.0641, 1.1241, 1.0811, 1.0458, 1.0745)      # mean 1.0779, max - min 0.0783: bound 1.313
R_MEASURED_RUN = "profiles/temporal/temporal_report.jsonl (tools/temporal_report.py, 1x MI355X)"


def rel_mse_median(img, truth):
    return float(np.median(((img.astype(np.float64) - truth) ** 2 / (truth.astype(np.float64) ** 2 + 1e-2)).mean(axis=-1)))


def test_orbit_history_improves_the_denoised_frame(device):
    """r was measured as R_ORBIT_MEASURED; this run's seeds are the report's, another machine's rounding aside"""
    hs, ds, seq = rendered_sequence("random_spheres_demo", 256, 144, 8, 8)
    try:
        truth, _ = ds.render(seq[-1][0], hs.params(256, 8192, 50, seed=77, height=144))
        shares = []
        with ds.temporal(256, 144) as t:
            for cam, g in seq:
                color, se, _, _ = run_frame(t, cam, g, want_history=False)
                shares.append(t.info().pixels_with_history / (256 * 144))
        g = seq[-1][1]
        alone = rel_mse(ds.denoise(g["color"], g["stderr3"], g["albedo"], g["normal"], g["depth"])[0], truth)
        both = rel_mse(ds.denoise(color, se, g["albedo"], g["normal"], g["depth"])[0], truth)
        print(f"relMSE denoised alone {alone:.5f} accumulated+denoised {both:.5f} ratio {both / alone:.4f}; history shares {shares}")
        assert min(shares[1:]) >= 0.90, shares           # a condition, not a measurement: the reprojection finds its history
        assert both < alone
        assert both / alone <= 1.0 - (1.0 - R_ORBIT_MEASURED) / 2.0, (both / alone, R_ORBIT_MEASURED)
    finally:
        ds.close()
        hs.close()


def test_fixed_camera_accumulation_is_a_32_spp_estimator(device):
    hs, ds, seq = rendered_sequence("cornell_box", 128, 128, 8, 4, fixed=True)
    try:
        cam = seq[0][0]
        truth, _ = ds.render(cam, hs.params(128, 8192, 50, seed=77, height=128))
        with ds.temporal(128, 128) as t:
            for cam_i, g in seq:
                color = run_frame(t, cam_i, g, want_history=False)[0]
        one, _ = ds.render(cam, hs.params(128, 32, 50, seed=1005, height=128))
        a, b = rel_mse(color, truth), rel_mse(one, truth)
        mean = sum(R_FIXED_MEASURED) / len(R_FIXED_MEASURED)
        spread = max(R_FIXED_MEASURED) - min(R_FIXED_MEASURED)
        print(f"relMSE accumulated 8 x 4 spp {a:.5f}, one 32-spp frame {b:.5f}, ratio {a / b:.4f}; bound {mean + 3 * spread:.4f}")
        assert a / b <= mean + 3.0 * spread, (a / b, R_FIXED_MEASURED)
        am, bm = rel_mse_median(color, truth), rel_mse_median(one, truth)
        mean = sum(R_FIXED_MEDIAN_MEASURED) / len(R_FIXED_MEDIAN_MEASURED)
        spread = max(R_FIXED_MEDIAN_MEASURED) - min(R_FIXED_MEDIAN_MEASURED)
        print(f"median over pixels: accumulated {am:.5f}, one 32-spp frame {bm:.5f}, ratio {am / bm:.4f}; bound {mean + 3 * spread:.4f}")
        assert am / bm <= mean + 3.0 * spread, (am / bm, R_FIXED_MEDIAN_MEASURED)
    finally:
        ds.close()
        hs.close()
