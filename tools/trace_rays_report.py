"""Cost of ray queries (vk_trace_rays) next to the first-hit pass (vk_render_aov) of the same frame.  Writes profiles/rays/report.jsonl
(one JSON line per batch, a summary line per frame, an autofocus line per frame) and prints the same lines.

    python tools/trace_rays_report.py [--repeats 5] [--cases c2,cornell,final] [--out profiles/rays/report.jsonl]

Frames: those of tools/aov_throughput.py — C2's scene (InOneWeekend random spheres) at 1920x1080, cornell_box at 900x900, final_scene at
800x800.  Rays: the primary rays of the pixel centres through the lens centre (the rays vk_temporal reconstructs), one per pixel, in three
orders — the 8x8 tiles of the first-hit kernel (a wave's 64 rays are one tile), row-major, and a seeded random permutation — and the
mirror-reflected rays from the tile-ordered batch's hits, an incoherent secondary batch.  Each batch: kernel ms (HIP events around the
launches, vk_stats.kernel_ms) as the median of --repeats calls after a warm-up, interleaved in the same process with a 1-spp
vk_render_aov call of the same frame; rays per second; the ratio of the time per ray to the first-hit kernel's time per primary ray.
The first-hit kernel's rays are jittered and pass through the lens, so the two walks are comparable, not identical.  The autofocus line:
the centre ray's t |d| next to the builder's focus distance.  For a kernel-level breakdown run it under `rocprofv3 --kernel-trace
--stats -- python tools/trace_rays_report.py ...` in a run of its own (trace_rays_kernel and aov_kernel in the stats)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vecchio_amd import DeviceScene, HostScene  # noqa: E402
from vecchio_amd.scene import make_rays  # noqa: E402

CASES = {"c2": ("random_spheres_iow", 1920, 1080), "cornell": ("cornell_box", 900, 900), "final": ("final_scene", 800, 800)}
f32 = np.float32


def vec(a):
    return f32(list(a))


def primary_rays(cam, w, h):
    """(h, w) rays of the pixel centres through the lens centre, f32 as the kernels compute them"""
    ys, xs = np.mgrid[0:h, 0:w]
    s = ((xs.astype(f32) + f32(0.5)) / f32(w - 1))[..., None]
    t = ((ys.astype(f32) + f32(0.5)) / f32(h - 1))[..., None]
    d = ((vec(cam.lower_left_corner) + vec(cam.horizontal) * s) + vec(cam.vertical) * t) - vec(cam.origin)
    o = np.broadcast_to(vec(cam.origin), d.shape)
    return make_rays(o, d, float(cam.time0)).reshape(h, w)


def tile_order(w, h):
    """pixel indices tile by tile (8x8, row-major tiles, row-major inside a tile): the first-hit kernel's lane order"""
    ys, xs = np.mgrid[0:h, 0:w]
    key = ((ys // 8) * ((w + 7) // 8) + xs // 8) * 64 + (ys % 8) * 8 + xs % 8
    return np.argsort(key.reshape(-1), kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays", "report.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for key in args.cases.split(","):
        name, w, h = CASES[key]
        hs = HostScene(name, 1)
        cam = hs.next_camera()
        ds = DeviceScene(hs.desc)
        try:
            pa = hs.params(w, 1, 50, height=h)
            rays = primary_rays(cam, w, h).reshape(-1)
            orders = {"tile": tile_order(w, h), "row": np.arange(w * h), "random": np.random.default_rng(1).permutation(w * h)}
            batches = {k: np.ascontiguousarray(rays[o]) for k, o in orders.items()}
            first = ds.trace_rays(batches["tile"], seed=1)
            hit = first["hit"] == 1
            d, n = batches["tile"]["direction"][hit], first["normal"][hit]
            refl = (d - f32(2) * (d * n).sum(1, keepdims=True).astype(f32) * n).astype(f32)
            batches["secondary"] = make_rays(first["p"][hit], refl, float(cam.time0))
            ds.render_aov(cam, pa, want=("depth",))                      # warm-up
            for b in batches.values():
                ds.trace_rays(b, seed=1)
            times = {k: [] for k in batches}
            aov = []
            for _ in range(args.repeats):                                # interleaved: one first-hit call, then one call per batch
                aov.append(ds.render_aov(cam, pa)[1].kernel_ms)
                for k, b in batches.items():
                    times[k].append(ds.trace_rays(b, seed=1, return_stats=True)[1].kernel_ms)
            aov_ms = statistics.median(aov)
            aov_ns = aov_ms * 1e6 / (w * h)
            ratios = {}
            for k, b in batches.items():
                ms = statistics.median(times[k])
                ratios[k] = round(ms * 1e6 / len(b) / aov_ns, 3)
                emit({"case": key, "scene": name, "width": w, "height": h, "batch": k, "rays": len(b), "kernel_ms": round(ms, 4),
                      "kernel_ms_all": [round(t, 4) for t in times[k]], "grays_per_s": round(len(b) / ms / 1e6, 3),
                      "ns_per_ray": round(ms * 1e6 / len(b), 3), "ratio_to_aov_per_ray": ratios[k]})
            emit({"case": key, "scene": name, "summary": True, "aov_1spp_kernel_ms": round(aov_ms, 4),
                  "aov_kernel_ms_all": [round(t, 4) for t in aov], "aov_ns_per_ray": round(aov_ns, 3), "hits_of_tile_batch": int(hit.sum()),
                  "ratio_to_aov_per_ray": ratios, "tile_order_within_2x": ratios["tile"] <= 2.0})
            # autofocus: the distance under the image centre, next to the distance the builder focused at (|horizontal| = 2 half_width focus,
            # |vertical| = 2 half_height focus: focus = |lower_left_corner + horizontal / 2 + vertical / 2 - origin| along -w)
            o = vec(cam.origin)
            c = vec(cam.lower_left_corner) + f32(0.5) * vec(cam.horizontal) + f32(0.5) * vec(cam.vertical) - o
            hc = ds.trace_rays(make_rays([o], [c], float(cam.time0)))[0]
            emit({"case": key, "scene": name, "autofocus": True, "centre_hit": int(hc["hit"]),
                  "centre_distance": (float(hc["t"]) * float(np.linalg.norm(c))) if hc["hit"] else None,
                  "builder_focus_dist": float(np.linalg.norm(c)), "object": int(hc["object"])})
        finally:
            ds.close()
            hs.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
