"""Probe queries (vk_trace_probes): the cost of the call next to vk_trace_radiance on the same rays, and the Cornell box's centre probe.
Writes profiles/probes/report.jsonl (one JSON line per frame, one for the centre probe) and prints the same lines.

    python tools/probes_report.py [--repeats 3] [--cases c2,cornell,final,centre] [--spp 64] [--out profiles/probes/report.jsonl]

Probe sets.  Frames: those of tools/trace_rays_report.py — C2's scene, cornell_box, final_scene.  Probes: a regular 64 x 64 grid in the
horizontal plane through the middle of the scene's bounds as the frame's camera sees them: the bounds of the first hits of a 96 x 54
frame of pixel-centre primary rays (vk_trace_rays), x and z cut to their 5th..95th percentile so that a ground that runs to the horizon
does not decide them.  --spp samples per probe.
Timing.  Interleaved in one process after a warm-up, --repeats times: vk_trace_probes, and vk_trace_radiance on the replayed rays — one
ray per (probe, sample), from the probe along the direction the probe query draws for that sample (taken from the per-sample hook), one
sample each.  Both calls trace the same rays; the radiance query continues other streams behind them, so the ratio compares rates: what
the direction drawn twice and the 27 LDS atomics of a sample cost against a ray load.  Kernel milliseconds are vk_stats.kernel_ms; the
median of the repeats is reported with every value kept.  Nothing passes or fails.  Each case is a timed step of its own: a child process
under a time limit; after one fails no further one is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = 300
GRID = 64
f32 = np.float32


def probe_grid(ds, cam):
    """the GRID x GRID probes of a frame (see above)"""
    from trace_rays_report import primary_rays
    from vecchio_amd.scene import make_probes
    hits = ds.trace_rays(primary_rays(cam, 96, 54).reshape(-1), 2, 0)
    p = hits["p"][(hits["hit"] == 1) & np.isfinite(hits["p"]).all(1)].astype(np.float64)
    (x0, x1), (z0, z1) = np.percentile(p[:, 0], [5, 95]), np.percentile(p[:, 2], [5, 95])
    y = 0.5 * (p[:, 1].min() + p[:, 1].max())
    zs, xs = np.mgrid[0:GRID, 0:GRID]
    pos = np.stack([x0 + (xs + 0.5) / GRID * (x1 - x0), np.full((GRID, GRID), y), z0 + (zs + 0.5) / GRID * (z1 - z0)], -1)
    return make_probes(pos.reshape(-1, 3).astype(f32), float(cam.time0)), (x0, x1, y, z0, z1)


def frame(key, repeats, spp):
    from trace_rays_report import CASES
    from vecchio_amd import DeviceScene, HostScene
    from vecchio_amd.scene import make_rays
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        probes, where = probe_grid(ds, cam)
        n = len(probes)
        kw = dict(seed=2, first_index=0, max_depth=50, integrator=hs.integrator, background=hs.background,
                  background_color=hs.background_color)
        # the replayed rays: the direction of every sample (drawing it does not depend on max_depth)
        _, dirs = ds.debug_probe_samples(probes, **dict(kw, samples_per_ray=spp, max_depth=1))
        replay = make_rays(np.repeat(probes["origin"], spp, 0), dirs[..., :3].reshape(-1, 3), np.repeat(probes["time"], spp))
        a, b = np.zeros((n, 9, 3), f32), np.zeros((n * spp, 3), f32)
        pkw, rkw = dict(kw, samples_per_ray=spp), dict(kw, samples_per_ray=1)
        ds.trace_probes(probes, out=a, **pkw)                           # warm-up
        ds.trace_radiance(replay, out=b, **rkw)
        ms_p, ms_r = [], []
        for _ in range(repeats):                                        # interleaved
            _, st = ds.trace_probes(probes, out=a, return_stats=True, **pkw)
            ms_p.append(st.kernel_ms)
            _, st = ds.trace_radiance(replay, out=b, return_stats=True, **rkw)
            ms_r.append(st.kernel_ms)
        qp, qr = statistics.median(ms_p), statistics.median(ms_r)
        s = n * spp
        print(json.dumps({"case": key, "scene": name, "probes": n, "spp": spp, "plane": [round(float(v), 3) for v in where],
                          "probes_ms": round(qp, 3), "probes_msamples_per_s": round(s / qp / 1e3, 1),
                          "probes_ms_all": [round(x, 3) for x in ms_p],
                          "radiance_ms": round(qr, 3), "radiance_msamples_per_s": round(s / qr / 1e3, 1),
                          "radiance_ms_all": [round(x, 3) for x in ms_r],
                          "probes_rate_over_radiance_rate": round(qr / qp, 4), "sh0_mean": round(float(a[:, 0].mean()), 5),
                          "radiance_mean": round(float(b.mean()), 5), "finite_share": round(float(np.isfinite(a).all((1, 2)).mean()), 6)}),
              flush=True)
    finally:
        ds.close()
        hs.close()


def centre(spp):
    """the probe in the middle of the Cornell box: its 27 coefficients and what vk_probe_eval makes of them for the six axis normals"""
    from vecchio_amd import DeviceScene, HostScene
    from vecchio_amd.scene import make_probes, probe_eval
    hs = HostScene("cornell_box", 1)
    ds = DeviceScene(hs.desc)
    try:
        sh, st = ds.trace_probes(make_probes([[278.0, 278.0, 278.0]]), seed=2, samples_per_ray=spp, max_depth=50, integrator=hs.integrator,
                                 background=hs.background, background_color=hs.background_color, return_stats=True)
        axes = {"+x": [1, 0, 0], "-x": [-1, 0, 0], "+y": [0, 1, 0], "-y": [0, -1, 0], "+z": [0, 0, 1], "-z": [0, 0, -1]}
        print(json.dumps({"case": "centre", "scene": "cornell_box", "position": [278.0, 278.0, 278.0], "spp": spp,
                          "sh": [[round(float(v), 6) for v in row] for row in sh[0]],
                          "irradiance_over_pi": {k: [round(float(v), 5) for v in probe_eval(sh[0], n, 1)] for k, n in axes.items()},
                          "radiance": {k: [round(float(v), 5) for v in probe_eval(sh[0], n, 0)] for k, n in axes.items()},
                          "clamped_samples": int(st.clamped_samples)}), flush=True)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final,centre")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probes", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its lines")
    args = ap.parse_args()
    if args.child:
        if args.child == "centre":
            centre(4096)
        else:
            frame(args.child, args.repeats, args.spp)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats), "--spp",
                                str(args.spp), "--out", args.out], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"case {key} ran into its time limit of {STEP_LIMIT_S} s; nothing further is started", file=sys.stderr)
            status = 1
            break
        got = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
        lines += got
        print("\n".join(got), flush=True)
        if r.returncode != 0:
            print(f"case {key} ended with status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", file=sys.stderr)
            status = 1
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
