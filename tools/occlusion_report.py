"""Cost of occlusion queries (vk_trace_occluded_device) next to the closest-hit query (vk_trace_rays_device) on the same rays and next to
the one-ray-per-lane form of the occlusion kernel.  Writes profiles/occlusion/report.jsonl (one JSON line per batch, the k x t sweep of
the refill form per frame) and prints the same lines.

    python tools/occlusion_report.py [--repeats 5] [--cases c2,cornell,final] [--out profiles/occlusion/report.jsonl]

Frames: those of tools/trace_rays_report.py — C2's scene at 1920x1080, cornell_box at 900x900, final_scene at 800x800.  Batches per frame:
the pixel-centre primary rays in tile order and in a seeded random order; a shadow batch from the first-hit points to a fixed point light
above the scene (origin p, direction light - p, tmax 1); and a batch that interleaves immediate hits (the primary ray restarted just before
its hit) with misses (the primary ray cut at half its hit distance).  Per batch, interleaved in one process after a warm-up: the
milliseconds (HIP events around one call, median of --repeats) and rays per second of vk_trace_occluded_device, of the debug library's
hook in its one-ray-per-lane form and in the refill form, and of vk_trace_rays_device, whose --repeats timings also give the run-to-run
spread ((max - min) / median) that the other differences are read against.  The sweep: the refill form's k (rays per lane of a wave's
block) x t (idle lanes that send a wave back to the claim) on the random-order batch.  Each frame is a timed step of its own: a child
process under a time limit; after one fails no further one is started."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIGHTS = {"c2": (0.0, 20.0, 0.0), "cornell": (278.0, 500.0, 278.0), "final": (278.0, 500.0, 278.0)}
SWEEP_K = (1, 2, 4, 8, 16, 32)
SWEEP_T = (1, 8, 16, 32, 64)
STEP_LIMIT_S = 240
f32 = np.float32


def frame(key, repeats):
    import torch
    torch.cuda.init()             # (before the library: torch's wheel carries its own HIP runtime)
    from trace_rays_report import CASES, primary_rays, tile_order
    from vecchio_amd import DeviceScene, HostScene, ffi
    from vecchio_amd.scene import make_rays
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    dbg = ffi.load_debug_lib()
    ds, dd = DeviceScene(hs.desc), DeviceScene(hs.desc, lib=dbg)
    out = []
    try:
        rays = primary_rays(cam, w, h).reshape(-1)
        tile = np.ascontiguousarray(rays[tile_order(w, h)])
        rnd = np.ascontiguousarray(rays[np.random.default_rng(1).permutation(w * h)])
        first = ds.trace_rays(rnd, seed=1)
        hit = first["hit"] == 1
        p, t = first["p"][hit], first["t"][hit]
        batches = {"tile": tile, "random": rnd,
                   "shadow": make_rays(p, f32(LIGHTS[key]) - p, float(cam.time0), 1.0)}
        o, d = rnd["origin"][hit], rnd["direction"][hit]
        near = make_rays(o + d * (f32(0.99) * t)[:, None], d, float(cam.time0))
        cut = make_rays(o, d, float(cam.time0), f32(0.5) * t)
        mixed = np.empty(2 * len(near), near.dtype)
        mixed[0::2], mixed[1::2] = near, cut
        batches["interleaved"] = mixed
        tp = ffi.TraceParams(1, 0, 0, 0)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for bname, b in batches.items():
            n = len(b)
            d_rays = torch.from_numpy(b.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
            d_occ = torch.empty((n,), dtype=torch.uint8, device="cuda:0")
            d_hits = torch.empty((n, 16), dtype=torch.int32, device="cuda:0")

            def hook(refill, k, t):
                st = dbg.vk_debug_trace_occluded_device(dd._h, C.byref(tp), C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_occ.data_ptr()),
                                                        None, refill, k, t)
                assert st == ffi.VK_OK, dbg.vk_last_error()

            calls = {"occluded": lambda: ds.trace_occluded(d_rays, 1, 0, out=d_occ),
                     "plain_form": lambda: hook(0, 0, 0),
                     "refill_form": lambda: hook(1, 8, 16),
                     "trace_rays": lambda: ds.trace_rays(d_rays, 1, 0, out=d_hits)}
            for fn in calls.values():                       # warm-up
                fn()
            torch.cuda.synchronize()
            occluded = int(d_occ.sum().item())
            ms = {k: [] for k in calls}
            for _ in range(repeats):                        # interleaved
                for k, fn in calls.items():
                    ms[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in ms.items()}
            rec = {"case": key, "scene": name, "width": w, "height": h, "batch": bname, "rays": n, "occluded": occluded,
                   "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                   "grays_per_s": {k: round(n / v / 1e6, 3) for k, v in med.items()},
                   "trace_rays_spread": round((max(ms["trace_rays"]) - min(ms["trace_rays"])) / med["trace_rays"], 4),
                   "occluded_over_trace_rays": round(med["occluded"] / med["trace_rays"], 4),
                   "refill_over_plain": round(med["refill_form"] / med["plain_form"], 4)}
            out.append(rec)
            print(json.dumps(rec), flush=True)
            if bname == "random":
                sweep = {}
                for k in SWEEP_K:
                    for t in SWEEP_T:
                        hook(1, k, t)
                        torch.cuda.synchronize()
                        sweep[f"k{k}_t{t}"] = round(statistics.median(timed(lambda: hook(1, k, t)) for _ in range(3)), 4)
                plain = round(statistics.median(timed(lambda: hook(0, 0, 0)) for _ in range(3)), 4)
                rec = {"case": key, "scene": name, "sweep": True, "batch": bname, "rays": n, "refill_ms": sweep, "plain_ms": plain}
                out.append(rec)
                print(json.dumps(rec), flush=True)
    finally:
        ds.close()
        dd.close()
        hs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one frame and print its lines")
    args = ap.parse_args()
    if args.child:
        frame(args.child, args.repeats)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"frame {key} ran into its time limit of {STEP_LIMIT_S} s; nothing further is started", file=sys.stderr)
            status = 1
            break
        got = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
        lines += got
        print("\n".join(got), flush=True)
        if r.returncode != 0:
            print(f"frame {key} ended with status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", file=sys.stderr)
            status = 1
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
