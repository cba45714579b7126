"""What the ID mattes (vk_render_mattes) cost, on the GPU.  One JSON line per case.

    python tools/mattes_report.py [--repeats 3] [--out profiles/mattes/report.jsonl]

The three report frames — C2's scene at 1920x1080, cornell_box at 900x900, final_scene at 800x800 — at 16 samples, seed 5: HIP-event
kernel time of vk_render_mattes for both kinds at ranks 4 and 8, next to vk_render_aov of the same frame and samples (the same walk, in
the same library), the calls interleaved, --repeats repetitions behind a warm-up of each: the median, and max - min as the spread.  Also
the share of the frame's pixels with overflow for each kind and rank.  Nothing is measured on import."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vecchio_amd import DeviceScene, HostScene, ffi  # noqa: E402

FRAMES = {"c2": ("random_spheres_iow", 1920, 1080), "cornell": ("cornell_box", 900, 900), "final": ("final_scene", 800, 800)}
KINDS = {"object": ffi.VK_MATTE_OBJECT, "material": ffi.VK_MATTE_MATERIAL}
RANKS = (4, 8)
SPP = 16


def frame_rows(key, args, emit):
    name, w, h = FRAMES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        p = hs.params(w, SPP, 50, seed=5, height=h)
        cases = [(kn, r) for kn in KINDS for r in RANKS]
        ms = {c: [] for c in cases}
        ms["aov"] = []
        share = {}
        bufs = {r: (np.zeros((h, w, r), np.uint32), np.zeros((h, w, r), np.uint32), np.zeros((h, w), np.uint32)) for r in RANKS}
        aov_out = None
        for rep in range(args.repeats + 1):                   # rep 0 = the warm-up of every call
            aov_out, st = ds.render_aov(cam, p, out=aov_out)
            if rep:
                ms["aov"].append(st.kernel_ms)
            for kn, r in cases:
                ids, counts, over, st = ds.render_mattes(cam, p, 0, KINDS[kn], r, out=bufs[r], return_stats=True)
                if rep:
                    ms[(kn, r)].append(st.kernel_ms)
                else:
                    assert (counts.sum(-1, dtype=np.uint64) + over == SPP).all()
                    share[(kn, r)] = float((over != 0).mean())
        aov = statistics.median(ms["aov"])
        emit({"case": key, "scene": name, "width": w, "height": h, "spp": SPP, "call": "vk_render_aov", "kernel_ms": round(aov, 4),
              "spread_ms": round(max(ms["aov"]) - min(ms["aov"]), 4), "repeats": args.repeats})
        for kn, r in cases:
            med = statistics.median(ms[(kn, r)])
            emit({"case": key, "scene": name, "width": w, "height": h, "spp": SPP, "call": "vk_render_mattes", "kind": kn, "ranks": r,
                  "kernel_ms": round(med, 4), "spread_ms": round(max(ms[(kn, r)]) - min(ms[(kn, r)]), 4), "ratio_to_aov": round(med / aov, 4),
                  "overflow_pixel_share": round(share[(kn, r)], 6), "repeats": args.repeats})
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for key in FRAMES:
        frame_rows(key, args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
