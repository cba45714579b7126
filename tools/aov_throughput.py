"""Cost of the first-hit buffers (vk_render_aov: albedo, normal, depth, coverage) next to the radiance frame they go with.  One JSON line
per case: the AOV kernel time (HIP events, median of --repeats calls after one warm-up), primary rays per second, and the ratio to the same
scene's vk_render frame time (kernel time of one frame after a warm-up frame, at the frame's own samples per pixel).

    python tools/aov_throughput.py [--repeats 5] [--cases c2,cornell,final]

Cases: C2's scene (InOneWeekend random spheres) at 1920x1080 with 16 AOV samples against its 1024-spp frame; cornell_box at 900x900 and
final_scene at 800x800 with 16 samples, against frames of --frame-spp samples.  For a kernel-level breakdown run it under
`rocprofv3 --kernel-trace --stats -- python tools/aov_throughput.py ...` in a run of its own (aov_kernel in the stats)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vecchio_amd import DeviceScene, HostScene  # noqa: E402

CASES = {"c2": ("random_spheres_iow", 1920, 1080, 1024), "cornell": ("cornell_box", 900, 900, None), "final": ("final_scene", 800, 800, None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--aov-spp", type=int, default=16)
    ap.add_argument("--frame-spp", type=int, default=256, help="samples per pixel of the reference frame of cornell / final")
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    for key in args.cases.split(","):
        name, w, h, frame_spp = CASES[key]
        frame_spp = frame_spp or args.frame_spp
        hs = HostScene(name, 1)
        cam = hs.next_camera()
        ds = DeviceScene(hs.desc)
        try:
            pa = hs.params(w, args.aov_spp, args.depth, height=h)
            ds.render_aov(cam, pa)                                       # warm-up
            times = [ds.render_aov(cam, pa)[1].kernel_ms for _ in range(args.repeats)]
            ms = statistics.median(times)
            pf = hs.params(w, frame_spp, args.depth, height=h)
            ds.render(cam, pf)                                           # warm-up
            frame_ms = ds.render(cam, pf)[1].kernel_ms
            rays = w * h * args.aov_spp
            print(json.dumps({"case": key, "scene": name, "width": w, "height": h, "aov_spp": args.aov_spp, "aov_kernel_ms": round(ms, 3),
                              "aov_kernel_ms_all": [round(t, 3) for t in times], "grays_per_s": round(rays / ms / 1e6, 3),
                              "frame_spp": frame_spp, "frame_kernel_ms": round(frame_ms, 2), "ratio_to_frame": round(ms / frame_ms, 4)}),
                  flush=True)
        finally:
            ds.close()
            hs.close()


if __name__ == "__main__":
    main()
