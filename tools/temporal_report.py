"""What temporal accumulation (vk_temporal_*) costs and what it buys, on the GPU.  One JSON line per case on stdout and in --out
(default profiles/temporal/temporal_report.jsonl), which a run starts afresh: the file is the record of one run.

    python tools/temporal_report.py [--repeats 7] [--part throughput|orbit|fixed|all] [--sweep] [--scenes random_spheres_demo,bowser_demo]

throughput: C2's scene at 1920x1080, cornell_box at 900x900, final_scene at 800x800.  Inputs: an 8-spp progressive frame in 2 windows, its
  standard error, AOVs at 8 spp.  The HIP-event time of one vk_temporal_accumulate call with every input and output, on a frame that has
  history everywhere (the same camera again: every pixel fetches four taps), median of --repeats after a warm-up; the default five-level
  vk_denoise call on the same inputs in the same run, the same way; the achieved GB/s against 176 bytes per pixel (52 in, 48 of history
  read, 48 written, 28 out).
orbit: an orbiting scene at 256x144 under its own RotatingCamera, 8 frames at 8 spp (2 windows, AOVs at 8 spp, seed 5 + frame): relative
  MSE mean((x - t)^2 / (t^2 + 0.01)) against vk_render at 8192 spp of frame 8's camera with seed 77, of frame 8 noisy, denoised alone,
  accumulated, and accumulated then denoised; the ratio tests/test_gpu_temporal.py pins is accumulated+denoised / denoised alone.  Per
  frame the share of pixels that took the history branch.  --sweep: the same over a grid of parameters.
fixed: cornell_box 128x128 under its fixed camera, 8 frames at 4 spp (2 windows): the accumulated frame 8 against one 32-spp vk_render
  frame, both against 8192 spp with seed 77, over 5 seed sets (frame seeds 5 + 100 k + frame, the 32-spp frame 1005 + 100 k).  Next to
  the relative MSE (a mean over pixels, which a few outlying pixels of a 32-spp Cornell frame dominate) the median over the pixels of
  the same per-pixel quantity (its mean over the three components), which measures the bulk of the pixels."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vecchio_amd import DeviceScene, HostScene  # noqa: E402

THROUGHPUT = {"c2": ("random_spheres_iow", 1920, 1080), "cornell": ("cornell_box", 900, 900), "final": ("final_scene", 800, 800)}
BYTES_PER_PIXEL = 52 + 48 + 48 + 28
# (max_history >= the number of frames is the default by construction)
SWEEP = [dict()] + [dict(max_history=v) for v in (2, 4, 6)] + [dict(depth_tol=v) for v in (0.005, 0.01, 0.05, 0.1)] + \
    [dict(normal_cos_min=v) for v in (0.5, 0.8, 0.95, 0.99)]
OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def frame(hs, ds, cam, w, h, spp, seed, windows=2):
    p = hs.params(w, spp, 50, seed=seed, height=h)
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(windows):
            img, _ = pr.step(spp // windows)
        se = pr.stderr()
    aov, _ = ds.render_aov(cam, p)
    return dict(color=img.copy(), stderr=se, albedo=aov["albedo"], normal=aov["normal"], depth=aov["depth"])


def rel_mse(img, truth):
    return float(np.mean((img.astype(np.float64) - truth) ** 2 / (truth.astype(np.float64) ** 2 + 1e-2)))


def rel_mse_median(img, truth):
    per_pixel = ((img.astype(np.float64) - truth) ** 2 / (truth.astype(np.float64) ** 2 + 1e-2)).mean(axis=-1)
    return float(np.median(per_pixel))


def denoise(ds, color, se, g):
    return ds.denoise(color, se, g["albedo"], g["normal"], g["depth"])


def throughput(args):
    for key in args.cases.split(","):
        name, w, h = THROUGHPUT[key]
        hs = HostScene(name, 1)
        cam = hs.next_camera()
        ds = DeviceScene(hs.desc)
        try:
            g = frame(hs, ds, cam, w, h, 8, 5)
            with ds.temporal(w, h) as t:
                ms = []
                for rep in range(args.repeats + 2):               # the first frame has no history, the second is the warm-up
                    st = t.accumulate(cam, want_history=True, **g)[3]
                    if rep >= 2:
                        ms.append(st.kernel_ms)
                share = t.info().pixels_with_history / (w * h)
            denoise(ds, g["color"], g["stderr"], g)
            dn = [denoise(ds, g["color"], g["stderr"], g)[1].kernel_ms for _ in range(args.repeats)]
            acc_ms, dn_ms = statistics.median(ms), statistics.median(dn)
            emit({"part": "throughput", "case": key, "scene": name, "width": w, "height": h, "accumulate_ms": round(acc_ms, 4),
                  "accumulate_ms_all": [round(v, 4) for v in ms], "denoise_default_ms": round(dn_ms, 4),
                  "ratio_to_denoise": round(acc_ms / dn_ms, 4), "gb_per_s": round(w * h * BYTES_PER_PIXEL / (acc_ms * 1e-3) / 1e9, 1),
                  "pixels_with_history_share": round(share, 4), "repeats": args.repeats})
        finally:
            ds.close()
            hs.close()


def orbit(args):
    w, h, nframes, spp = 256, 144, 8, 8
    for name in args.scenes.split(","):
        hs = HostScene(name, 1)
        ds = DeviceScene(hs.desc)
        try:
            cams = [hs.next_camera() for _ in range(nframes)]
            frames = [frame(hs, ds, cams[i], w, h, spp, 5 + i) for i in range(nframes)]
            truth = ds.render(cams[-1], hs.params(w, 8192, 50, seed=77, height=h))[0]
            last = frames[-1]
            noisy = rel_mse(last["color"], truth)
            alone = rel_mse(denoise(ds, last["color"], last["stderr"], last)[0], truth)
            for over in (SWEEP if args.sweep else [dict()]):
                shares = []
                with ds.temporal(w, h, **over) as t:
                    for cam, g in zip(cams, frames):
                        color, se, _, _ = t.accumulate(cam, **g)
                        shares.append(round(t.info().pixels_with_history / (w * h), 4))
                acc = rel_mse(color, truth)
                both = rel_mse(denoise(ds, color, se, last)[0], truth)
                emit({"part": "orbit", "scene": name, "width": w, "height": h, "frames": nframes, "spp": spp, "params": over,
                      "relmse_noisy": round(noisy, 6), "relmse_denoised_alone": round(alone, 6), "relmse_accumulated": round(acc, 6),
                      "relmse_accumulated_denoised": round(both, 6), "ratio": round(both / alone, 4),
                      "ratio_accumulated_to_noisy": round(acc / noisy, 4), "history_share_per_frame": shares,
                      "history_share_min_frames_2_to_8": min(shares[1:])})
        finally:
            ds.close()
            hs.close()


def fixed(args):
    w = h = 128
    hs = HostScene("cornell_box", 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        truth = ds.render(cam, hs.params(w, 8192, 50, seed=77, height=h))[0]
        ratios, medians = [], []
        for k in range(5):
            with ds.temporal(w, h) as t:
                for i in range(8):
                    color, _, hist, _ = t.accumulate(cam, want_history=True, **frame(hs, ds, cam, w, h, 4, 5 + 100 * k + i))
                share = t.info().pixels_with_history / (w * h)
            one = ds.render(cam, hs.params(w, 32, 50, seed=1005 + 100 * k, height=h))[0]
            a, b = rel_mse(color, truth), rel_mse(one, truth)
            ratios.append(round(a / b, 4))
            am, bm = rel_mse_median(color, truth), rel_mse_median(one, truth)
            medians.append(round(am / bm, 4))
            emit({"part": "fixed", "scene": "cornell_box", "width": w, "height": h, "seed_set": k, "relmse_accumulated_8x4spp": round(a, 6),
                  "relmse_render_32spp": round(b, 6), "ratio": ratios[-1], "median_accumulated_8x4spp": round(am, 6), "median_render_32spp": round(bm, 6),
                  "ratio_median": medians[-1], "history_share_frame_8": round(share, 4),
                  "pixels_with_full_history_share": round(float((hist > 7.5).mean()), 4), "mean_history_length": round(float(hist.mean()), 3)})
        emit({"part": "fixed_summary", "ratios": ratios, "mean": round(statistics.mean(ratios), 4),
              "spread_max_minus_min": round(max(ratios) - min(ratios), 4), "ratios_median": medians,
              "mean_median": round(statistics.mean(medians), 4), "spread_median_max_minus_min": round(max(medians) - min(medians), 4)})
    finally:
        ds.close()
        hs.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("all", "throughput", "orbit", "fixed"))
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--scenes", default="random_spheres_demo,bowser_demo")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "temporal_report.jsonl"))
    args = ap.parse_args()
    OUT = args.out
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        open(OUT, "w").close()
    if args.part in ("all", "throughput"):
        throughput(args)
    if args.part in ("all", "orbit"):
        orbit(args)
    if args.part in ("all", "fixed"):
        fixed(args)


if __name__ == "__main__":
    main()
