"""Shade queries (vk_shade_hits): the cost of a bounce next to the walk that found its hits, next to a device copy of the bytes it moves,
and the whole wavefront loop next to vk_trace_radiance.  Writes profiles/shade/report.jsonl (one JSON line per frame) and prints them.

    python tools/shade_report.py [--repeats 3] [--cases c2,cornell,final] [--out profiles/shade/report.jsonl]

Frames: those of tools/trace_rays_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 — with the pixel-centre
primary rays, row-major, one path per ray, max_depth 50, the scene's own integrator and background.
The loop is vk_shade_hits' contract: fresh states, then vk_trace_rays and vk_shade_hits in turn on the paths still alive.  Per bounce,
after a warm-up of both calls, --repeats times interleaved in one process: vk_trace_rays on the bounce's rays, vk_shade_hits on the same
rays with those hits.  Kernel milliseconds are vk_stats.kernel_ms (device events around the launches, summed over a call's chunks; the
host-pointer calls' staging copies are outside them and are reported as the calls' wall seconds); the median of the repeats is reported
with every value kept.  A bounce's bytes are 240 an item (32 + 64 + 48 read, 96 written — a device copy of n bytes counted the same
way moves n / 2 in and n / 2 out); the copy is a device-to-device hipMemcpyAsync of that many bytes between two events, in the same
process, the same number of repeats.  vk_trace_radiance runs the same rays at 1 sample per ray, interleaved with nothing: its kernel
milliseconds stand next to the sum over the bounces of the loop's medians.  Nothing passes or fails.  Each frame is a timed step of its
own: a child process under a time limit; after one fails no further one is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = 420
ITEM_BYTES = 240
f32 = np.float32


def copy_ms(torch, nbytes, repeats):
    """a device-to-device copy of nbytes, timed between two events: every repeat's milliseconds"""
    n = max(16, nbytes // 2)                # nbytes moved in all: n read and n written
    a = torch.zeros(n, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def frame(key, repeats):
    import torch            # first: its wheel carries its own HIP runtime, which must be the one that initialises the device
    torch.cuda.init()
    from trace_rays_report import CASES, primary_rays
    from vecchio_amd import DeviceScene, HostScene, ffi
    from vecchio_amd.scene import make_path_states
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        rays = np.ascontiguousarray(primary_rays(cam, w, h).reshape(-1))
        n = len(rays)
        kw = dict(max_depth=50, integrator=hs.integrator, background=hs.background, background_color=hs.background_color)
        seed = 2
        states = make_path_states(n, seed, 0, 0)
        live = np.arange(n)
        acc = np.zeros((n, 3), f32)
        bounces = []
        while live.size:
            m = len(rays)
            fi = len(bounces) * n
            hits = ds.trace_rays(rays, seed, fi)                                    # warm-up of this shape, and the bounce's hits
            out = ds.shade_hits(rays, hits, states, **kw)
            ms_t, ms_s, wall_t, wall_s = [], [], [], []
            for _ in range(repeats):                                                # interleaved
                t0 = time.perf_counter()
                _, st = ds.trace_rays(rays, seed, fi, out=hits, return_stats=True)
                wall_t.append(time.perf_counter() - t0); ms_t.append(st.kernel_ms)
                t0 = time.perf_counter()
                _, st = ds.shade_hits(rays, hits, states, out=out, return_stats=True, **kw)
                wall_s.append(time.perf_counter() - t0); ms_s.append(st.kernel_ms)
            ms_c = copy_ms(torch, m * ITEM_BYTES, repeats)
            qt, qs, qc = statistics.median(ms_t), statistics.median(ms_s), statistics.median(ms_c)
            status = out["status"]
            bounces.append({"bounce": len(bounces) + 1, "items": m, "hit_share": round(float((hits["hit"] == 1).mean()), 4),
                            "scattered_share": round(float((status == ffi.VK_SHADE_SCATTERED).mean()), 4),
                            "trace_ms": round(qt, 4), "trace_ms_all": [round(x, 4) for x in ms_t],
                            "shade_ms": round(qs, 4), "shade_ms_all": [round(x, 4) for x in ms_s],
                            "shade_over_trace": round(qs / qt, 4),
                            "shade_gbytes_per_s": round(m * ITEM_BYTES / qs / 1e6, 1),
                            "copy_ms": round(qc, 4), "copy_ms_all": [round(x, 4) for x in ms_c],
                            "copy_gbytes_per_s": round(m * ITEM_BYTES / qc / 1e6, 1), "shade_over_copy": round(qs / qc, 3),
                            "trace_wall_s": round(statistics.median(wall_t), 4), "shade_wall_s": round(statistics.median(wall_s), 4)})
            acc[live] = out["state"]["acc"]
            go = status == ffi.VK_SHADE_SCATTERED
            live, rays, states = live[go], np.ascontiguousarray(out["next"][go]), np.ascontiguousarray(out["state"][go])
        # the radiance query on the same rays, 1 sample per ray
        rays0 = np.ascontiguousarray(primary_rays(cam, w, h).reshape(-1))
        rkw = dict(kw, seed=seed, first_index=0, samples_per_ray=1)
        rgb = ds.trace_radiance(rays0, **rkw)                                       # warm-up
        ms_r = []
        for _ in range(repeats):
            _, st = ds.trace_radiance(rays0, out=rgb, return_stats=True, **rkw)
            ms_r.append(st.kernel_ms)
        qr = statistics.median(ms_r)
        loop_t, loop_s = sum(b["trace_ms"] for b in bounces), sum(b["shade_ms"] for b in bounces)
        finite = np.isfinite(acc).all(1)
        # the contract, as far as the query's aggregation lets it show: without media the loop's radiance is the query's sample, which the
        # query drops when it is not finite and rounds to its 2^-26 fixed point
        same = None
        if not hs.desc.contents.n_media:
            mine = np.where(finite[:, None], acc, 0)
            same = round(float((np.abs(mine - rgb) <= np.maximum(2.0 ** -25, 1e-6 * np.abs(rgb))).all(1).mean()), 6)
        print(json.dumps({"case": key, "scene": name, "width": w, "height": h, "rays": n, "repeats": repeats, "n_bounces": len(bounces),
                          "loop_trace_ms": round(loop_t, 3), "loop_shade_ms": round(loop_s, 3), "loop_kernel_ms": round(loop_t + loop_s, 3),
                          "loop_wall_s": round(sum(b["trace_wall_s"] + b["shade_wall_s"] for b in bounces), 3),
                          "radiance_ms": round(qr, 3), "radiance_ms_all": [round(x, 3) for x in ms_r],
                          "loop_kernel_over_radiance": round((loop_t + loop_s) / qr, 4), "shade_share_of_loop_kernel": round(loop_s / (loop_t + loop_s), 4),
                          "share_of_rays_matching_radiance": same, "mean_radiance": round(float(acc[finite].mean()), 5),
                          "bounces": bounces}), flush=True)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its line")
    args = ap.parse_args()
    if args.child:
        frame(args.child, args.repeats)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats), "--out", args.out],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
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
