"""Adaptive progressive rendering (vk_progress_set_adaptive) on the C2 frame (InOneWeekend random spheres, 1920x1080, depth 50): a budget
of 1024 spp in 64-spp windows, non-adaptive and then adaptive for a few absolute tolerances (per component, standard error <= tol).
Prints one JSON line per step: active tiles (before the step), kernel ms, wall ms and the Msamples/s of the samples really rendered;
then one summary line per run: total time against the non-adaptive run, samples rendered, and the final per-pixel standard error's
quantiles (the largest component per pixel).

    python tools/adaptive_progress.py [--width 1920] [--spp 1024] [--window 64] [--tols 0.02,0.01,0.005]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vecchio_amd import DeviceScene, HostScene  # noqa: E402


def run(ds, cam, p, window, adaptive, label):
    out = np.zeros((p.height, p.width, 3), np.float32)
    with ds.progress(cam, p, stderr=True, adaptive=adaptive) as pr:
        t0 = time.perf_counter()
        total_samples, kms = 0, 0.0
        for j in range(p.samples_per_pixel // window):
            active = pr.tile_samples()[1].tiles_active
            s0 = time.perf_counter()
            _, st = pr.step(window, out=out)
            wall = time.perf_counter() - s0
            total_samples += st.samples
            kms += st.kernel_ms
            print(json.dumps({"run": label, "step": j + 1, "active_tiles": active, "kernel_ms": round(st.kernel_ms, 3),
                              "wall_ms": round(1e3 * wall, 3), "msamples": round(st.samples / 1e6, 2),
                              "kernel_msamples_per_s": round(st.samples / st.kernel_ms / 1e3, 1) if st.samples else 0.0}), flush=True)
        seconds = time.perf_counter() - t0
        tmap, inf = pr.tile_samples()
        se = pr.stderr().max(axis=2)
    q = {f"stderr_p{int(100 * f)}": round(float(np.quantile(se, f)), 5) for f in (0.5, 0.9, 0.99)}
    q["stderr_max"] = round(float(se.max()), 5)
    return seconds, kms, total_samples, inf, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="random_spheres_iow")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--tols", default="0.02,0.01,0.005")
    args = ap.parse_args()
    hs = HostScene(args.scene, 1)
    cam = hs.next_camera()
    p = hs.params(args.width, args.spp, args.depth)
    ds = DeviceScene(hs.desc)
    run(ds, cam, p, args.window, None, "warm-up")
    base = run(ds, cam, p, args.window, None, "plain")
    print(json.dumps({"run": "plain", "seconds": round(base[0], 3), "kernel_ms": round(base[1], 1), "gsamples": round(base[2] / 1e9, 3),
                      "msamples_per_s": round(base[2] / base[0] / 1e6, 1), **base[4]}), flush=True)
    for tol in [float(t) for t in args.tols.split(",")]:
        r = run(ds, cam, p, args.window, dict(abs_tol=tol, rel_tol=0.0, min_samples=0, min_steps=2), f"tol={tol}")
        print(json.dumps({"run": f"tol={tol}", "seconds": round(r[0], 3), "of_plain_time": round(r[0] / base[0], 3),
                          "kernel_ms": round(r[1], 1), "gsamples": round(r[2] / 1e9, 3), "of_plain_samples": round(r[2] / base[2], 3),
                          "msamples_per_s": round(r[2] / r[0] / 1e6, 1), "tiles_active_at_end": r[3].tiles_active,
                          "tiles_total": r[3].tiles_total, **r[4]}), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
