"""Cost of radiance queries (vk_trace_radiance) next to vk_render of the same frame on the same tree view.  Writes
profiles/radiance/report.jsonl (one JSON line per frame and ray order, one for the panorama) and prints the same lines.

    python tools/radiance_report.py [--repeats 3] [--cases c2,cornell,final] [--spp 16] [--out profiles/radiance/report.jsonl]

Frames: those of tools/trace_rays_report.py — C2's scene at 1920x1080, cornell_box at 900x900, final_scene at 800x800.  Rays: the
pixel-centre primary rays of the frame in tile order (8x8 tiles, vk_render's own order), in row-major order and in a seeded random order.
Per order, interleaved in one process after a warm-up: the kernel milliseconds (vk_stats.kernel_ms, summed over the call's chunks; median
of --repeats) and Msamples/s of vk_trace_radiance at --spp samples per ray, and of vk_render of the same frame at --spp samples per pixel
on a scene created with VK_SCENE_REFERENCE_TREE — the tree view the query walks.  The two do not compute the same samples (vk_render
jitters its rays, the query repeats the pixel centre); the ratio compares rates, nothing else.  The panorama: an equirectangular
2048x1024 image of C2's scene from the camera's origin, written as profiles/radiance/panorama_c2.pfm (not kept in the repository).
Each frame is a timed step of its own: a child process under a time limit; after one fails no further one is started."""
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
    """img (h, w, 3) float32, y = 0 the bottom row (PFM's own order)"""
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(img, "<f4").tobytes())


def frame(key, repeats, spp, out_dir):
    from trace_rays_report import CASES, primary_rays, tile_order
    from vecchio_amd import DeviceScene, HostScene, ffi
    from vecchio_amd.scene import make_rays
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    hs.desc.contents.flags = ffi.VK_SCENE_REFERENCE_TREE
    ds = DeviceScene(hs.desc)
    try:
        rays = primary_rays(cam, w, h).reshape(-1)
        orders = {"tile": np.ascontiguousarray(rays[tile_order(w, h)]), "row_major": rays,
                  "random": np.ascontiguousarray(rays[np.random.default_rng(1).permutation(w * h)])}
        p = hs.params(w, spp, 50, seed=2, height=h)
        kw = dict(seed=2, first_index=0, samples_per_ray=spp, max_depth=50, integrator=hs.integrator, background=hs.background,
                  background_color=hs.background_color)
        img = np.zeros((h, w, 3), f32)
        rgb = np.zeros((w * h, 3), f32)
        ds.render(cam, p, out=img)                                  # warm-up
        ds.trace_radiance(orders["tile"], out=rgb, **kw)
        for oname, b in orders.items():
            ms_q, ms_r = [], []
            for _ in range(repeats):                                # interleaved
                _, st = ds.trace_radiance(b, out=rgb, return_stats=True, **kw)
                ms_q.append(st.kernel_ms)
                _, st = ds.render(cam, p, out=img)
                ms_r.append(st.kernel_ms)
            q, r = statistics.median(ms_q), statistics.median(ms_r)
            n = w * h * spp
            rec = {"case": key, "scene": name, "width": w, "height": h, "spp": spp, "order": oname, "rays": w * h,
                   "query_ms": round(q, 3), "query_msamples_per_s": round(n / q / 1e3, 1), "query_ms_all": [round(x, 3) for x in ms_q],
                   "render_ms": round(r, 3), "render_msamples_per_s": round(n / r / 1e3, 1), "render_ms_all": [round(x, 3) for x in ms_r],
                   "query_rate_over_render_rate": round(r / q, 4), "query_mean": round(float(rgb.mean()), 5),
                   "render_mean": round(float(img.mean()), 5)}
            print(json.dumps(rec), flush=True)
        if key == "c2":
            pw, ph = 2048, 1024
            ys, xs = np.mgrid[0:ph, 0:pw]
            phi = ((xs + 0.5) / pw * 2.0 - 1.0) * np.pi
            theta = ((ys + 0.5) / ph - 0.5) * np.pi                  # row 0: straight down
            d = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta), -np.cos(theta) * np.cos(phi)], -1).astype(f32).reshape(-1, 3)
            pr = make_rays(np.tile(f32(list(cam.origin)), (pw * ph, 1)), d, float(cam.time0))
            pano, st = ds.trace_radiance(pr, return_stats=True, **kw)
            os.makedirs(out_dir, exist_ok=True)
            write_pfm(os.path.join(out_dir, "panorama_c2.pfm"), pano.reshape(ph, pw, 3))
            n = pw * ph * spp
            print(json.dumps({"case": "c2", "scene": name, "panorama": True, "width": pw, "height": ph, "spp": spp,
                              "query_ms": round(st.kernel_ms, 3), "query_msamples_per_s": round(n / st.kernel_ms / 1e3, 1),
                              "kernel_launches": st.kernel_launches, "finite": bool(np.isfinite(pano).all()),
                              "mean": round(float(pano.mean()), 5)}), flush=True)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one frame and print its lines")
    args = ap.parse_args()
    if args.child:
        frame(args.child, args.repeats, args.spp, os.path.dirname(os.path.abspath(args.out)))
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats), "--spp",
                                str(args.spp), "--out", args.out], capture_output=True, text=True, timeout=STEP_LIMIT_S)
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
