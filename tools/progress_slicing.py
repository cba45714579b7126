"""Cost of slicing a frame into progressive steps (vk_progress_*): the C2 frame (InOneWeekend random spheres, 1920x1080, depth 50) rendered
to 1024 spp in one vk_render call and as 1x1024, 4x256, 16x64 and 64x16 progressive steps.  Prints one JSON line per configuration:
Msamples/s over the whole frame (wall time of the blocking steps, the host copies of every preview included) and per step, the
kernel time (HIP events, the accumulate kernel included) and whether the final image is the one-shot frame bit for bit.

    python tools/progress_slicing.py [--width 1920] [--spp 1024] [--repeats 2]

For the accumulate kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python tools/progress_slicing.py ...` in a run of
its own (accumulate_resolve_kernel in the stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vecchio_amd import DeviceScene, HostScene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="random_spheres_iow")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--steps", default="1,4,16,64")
    ap.add_argument("--repeats", type=int, default=2, help="timed frames per configuration (after one warm-up frame)")
    args = ap.parse_args()
    hs = HostScene(args.scene, 1)
    cam = hs.next_camera()
    p = hs.params(args.width, args.spp, args.depth)
    ds = DeviceScene(hs.desc)
    out = np.zeros((p.height, p.width, 3), np.float32)

    def one_shot():
        t0 = time.perf_counter()
        _, st = ds.render(cam, p, out=out)
        return time.perf_counter() - t0, st.kernel_ms, st.samples

    one_shot()
    ref = out.copy()
    best = min(one_shot() for _ in range(args.repeats))
    base_rate = best[2] / best[0] / 1e6
    print(json.dumps({"config": "vk_render", "spp": args.spp, "seconds": round(best[0], 4), "kernel_ms": round(best[1], 3),
                      "msamples_per_s": round(base_rate, 1), "kernel_msamples_per_s": round(best[2] / best[1] / 1e3, 1)}), flush=True)
    for steps in [int(s) for s in args.steps.split(",")]:
        n = args.spp // steps
        runs = []
        for r in range(args.repeats + 1):
            with ds.progress(cam, p) as pr:
                t0 = time.perf_counter()
                kms, samples, per_step = 0.0, 0, []
                for _ in range(steps):
                    s0 = time.perf_counter()
                    _, st = pr.step(n, out=out)
                    per_step.append(time.perf_counter() - s0)
                    kms += st.kernel_ms
                    samples += st.samples
                runs.append((time.perf_counter() - t0, kms, samples, per_step))
        wall, kms, samples, per_step = min(runs[1:], key=lambda x: x[0])
        rate = samples / wall / 1e6
        print(json.dumps({"config": f"{steps}x{n}", "seconds": round(wall, 4), "kernel_ms": round(kms, 3),
                          "msamples_per_s": round(rate, 1), "of_one_shot": round(rate / base_rate, 3),
                          "ms_per_step_median": round(1e3 * float(np.median(per_step)), 3),
                          "kernel_ms_per_step": round(kms / steps, 3), "kernel_msamples_per_s": round(samples / kms / 1e3, 1),
                          "bit_identical": bool(np.array_equal(out.view(np.uint32), ref.view(np.uint32)))}), flush=True)
    ds.close()


if __name__ == "__main__":
    main()
