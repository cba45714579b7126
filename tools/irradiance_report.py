"""Irradiance queries (vk_trace_irradiance): a baked lightmap, and the cost of the call next to vk_trace_radiance on the same rays.  Writes
profiles/irradiance/report.jsonl (one JSON line for the lightmap, one per frame) and prints the same lines.

    python tools/irradiance_report.py [--repeats 3] [--cases lightmap,c2,cornell,final] [--spp 16] [--out profiles/irradiance/report.jsonl]

Lightmap: 256x256 texels on the floor of cornell_box (y = 0, x and z in 0..555, normal +y), 64 samples per texel, written as
profiles/irradiance/lightmap_cornell_floor.pfm (not kept in the repository) with its minimum, maximum and the share of finite texels.
Nothing is compared and nothing passes or fails.

Timing.  Frames: those of tools/trace_rays_report.py — C2's scene at 1920x1080, cornell_box at 900x900, final_scene at 800x800.  Points:
the first hits of the frame's pixel-centre primary rays (vk_trace_rays + points_from_hits: misses and medium hits left out), in
row-major order.  Interleaved in one process after a warm-up, --repeats times: vk_trace_irradiance at --spp samples per point, and
vk_trace_radiance at --spp samples per ray on the replayed rays — one ray per point, from the point along the direction the irradiance
query draws for its first sample (taken from the per-sample hook).  Kernel milliseconds are vk_stats.kernel_ms summed over a call's
chunks; the median of the repeats is reported with every value kept.  The two calls do not compute the same samples (the radiance
query repeats one direction, the irradiance query draws one per sample): the ratio compares rates, i.e. what the direction draw in the
refill and the less coherent first segments cost against a ray load.  Each case is a timed step of its own: a child process under a time
limit; after one fails no further one is started."""
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
f32 = np.float32


def write_pfm(path, img):
    """img (h, w, 3) float32, row 0 the bottom row (PFM's own order)"""
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(img, "<f4").tobytes())


def lightmap(out_dir):
    from vecchio_amd import DeviceScene, HostScene
    from vecchio_amd.scene import make_points
    hs = HostScene("cornell_box", 1)
    ds = DeviceScene(hs.desc)
    try:
        n, spp = 256, 64
        zs, xs = np.mgrid[0:n, 0:n]
        p = np.stack([(xs + 0.5) / n * 555.0, np.zeros((n, n)), (zs + 0.5) / n * 555.0], -1).astype(f32).reshape(-1, 3)
        pts = make_points(p, np.tile(f32([0, 1, 0]), (n * n, 1)))
        rgb, st = ds.trace_irradiance(pts, seed=2, samples_per_ray=spp, max_depth=50, integrator=hs.integrator, background=hs.background,
                                      background_color=hs.background_color, return_stats=True)
        os.makedirs(out_dir, exist_ok=True)
        write_pfm(os.path.join(out_dir, "lightmap_cornell_floor.pfm"), rgb.reshape(n, n, 3))
        print(json.dumps({"case": "lightmap", "scene": "cornell_box", "width": n, "height": n, "spp": spp,
                          "query_ms": round(st.kernel_ms, 3), "query_msamples_per_s": round(n * n * spp / st.kernel_ms / 1e3, 1),
                          "min": round(float(rgb.min()), 6), "max": round(float(rgb.max()), 6), "mean": round(float(rgb.mean()), 6),
                          "finite_share": round(float(np.isfinite(rgb).all(1).mean()), 6),
                          "clamped_samples": int(st.clamped_samples)}), flush=True)
    finally:
        ds.close()
        hs.close()


def frame(key, repeats, spp):
    from trace_rays_report import CASES, primary_rays
    from vecchio_amd import DeviceScene, HostScene
    from vecchio_amd.scene import make_rays, points_from_hits
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        rays = primary_rays(cam, w, h).reshape(-1)
        pts, _ = points_from_hits(ds.trace_rays(rays, 2, 0), float(cam.time0))
        n = len(pts)
        kw = dict(seed=2, first_index=0, max_depth=50, integrator=hs.integrator, background=hs.background,
                  background_color=hs.background_color)
        # the replayed rays: the direction of every point's first sample (drawing it does not depend on max_depth)
        _, dirs = ds.debug_irradiance_samples(pts, **dict(kw, samples_per_ray=1, max_depth=1))
        replay = make_rays(pts["origin"], dirs[:, 0, :3], pts["time"])
        a, b = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
        kw["samples_per_ray"] = spp
        ds.trace_irradiance(pts, out=a, **kw)                           # warm-up
        ds.trace_radiance(replay, out=b, **kw)
        ms_i, ms_r = [], []
        for _ in range(repeats):                                        # interleaved
            _, st = ds.trace_irradiance(pts, out=a, return_stats=True, **kw)
            ms_i.append(st.kernel_ms)
            _, st = ds.trace_radiance(replay, out=b, return_stats=True, **kw)
            ms_r.append(st.kernel_ms)
        qi, qr = statistics.median(ms_i), statistics.median(ms_r)
        s = n * spp
        print(json.dumps({"case": key, "scene": name, "width": w, "height": h, "spp": spp, "points": n, "pixels": w * h,
                          "irradiance_ms": round(qi, 3), "irradiance_msamples_per_s": round(s / qi / 1e3, 1),
                          "irradiance_ms_all": [round(x, 3) for x in ms_i],
                          "radiance_ms": round(qr, 3), "radiance_msamples_per_s": round(s / qr / 1e3, 1),
                          "radiance_ms_all": [round(x, 3) for x in ms_r],
                          "irradiance_rate_over_radiance_rate": round(qr / qi, 4), "irradiance_mean": round(float(a.mean()), 5),
                          "radiance_mean": round(float(b.mean()), 5)}), flush=True)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="lightmap,c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irradiance", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its lines")
    args = ap.parse_args()
    if args.child:
        if args.child == "lightmap":
            lightmap(os.path.dirname(os.path.abspath(args.out)))
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
