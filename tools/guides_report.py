"""What the specular guides (vk_render_guides) cost and what they buy, on the GPU.  One JSON line per case.

    python tools/guides_report.py [--part time,quality,temporal] [--repeats 5] [--out profiles/guides/report.jsonl]

time:    vk_render_guides at 16 samples and the defaults next to vk_render_aov in the same run, HIP-event kernel time, the two
         alternating, median of --repeats after a warm-up of each: C2's scene at 1920x1080, cornell_box at 900x900, final_scene at
         800x800.  With the mean `bounces` of the frame, the time per traced segment (1 + mean bounces segments per sample for the
         guides, 1 for the first hits) and, for C2, the share of a 1024-spp frame (64 x a timed 16-spp progressive step).
quality: the InOneWeekend frame of tools/denoise_report.py (256x144, 16 spp in 4 windows, reference vk_render at 8192 spp), denoised
         from vk_render_aov's guides and from vk_render_guides', relative MSE over the frame and over the delta pixels (bounces >= 0.5),
         for five seed sets: the ratios new / old and the spread of the whole-frame ratio.
temporal: the random_spheres_demo orbit of tools/temporal_report.py (256x144, 8 frames at 8 spp in 2 windows, frame seed 5 + frame,
         reference vk_render at 8192 spp of frame 8's camera with seed 77), accumulated (vk_temporal_*, defaults) and then denoised,
         once with vk_render_aov's albedo, normal and depth and once with vk_render_guides': relative MSE of frame 8 noisy, denoised
         alone, accumulated, accumulated and denoised, over the frame and over the delta pixels of frame 8, and the share of pixels
         with history per frame.
Nothing is measured on import."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vecchio_amd import DeviceScene, HostScene  # noqa: E402

TIME = {"c2": ("random_spheres_iow", 1920, 1080), "cornell": ("cornell_box", 900, 900), "final": ("final_scene", 800, 800)}
SEED_SETS = [(5, 77), (6, 78), (7, 79), (8, 80), (9, 81)]          # (frame seed, reference seed); the first is denoise_report's


def rel_mse(img, truth, mask=None):
    e = (img.astype(np.float64) - truth) ** 2 / (truth.astype(np.float64) ** 2 + 1e-2)
    return float(np.mean(e if mask is None else e[mask]))


def time_part(args, emit):
    for key, (name, w, h) in TIME.items():
        hs = HostScene(name, 1)
        cam = hs.next_camera()
        ds = DeviceScene(hs.desc)
        try:
            p = hs.params(w, 16, 50, seed=5, height=h)
            ms = {"aov": [], "guides": []}
            bounces = None
            for rep in range(args.repeats + 1):               # rep 0 = the warm-up of both
                _, st = ds.render_aov(cam, p, want=("albedo", "normal", "depth"))
                g, sg = ds.render_guides(cam, p, want=("albedo", "normal", "depth", "bounces"))
                bounces = float(g["bounces"].mean())
                if rep:
                    ms["aov"].append(st.kernel_ms)
                    ms["guides"].append(sg.kernel_ms)
            aov, gd = statistics.median(ms["aov"]), statistics.median(ms["guides"])
            row = {"part": "time", "case": key, "scene": name, "width": w, "height": h, "aov_ms": round(aov, 4), "guides_ms": round(gd, 4),
                   "mean_bounces": round(bounces, 4), "ms_per_segment_ratio": round(gd / (1.0 + bounces) / aov, 4), "repeats": args.repeats}
            if key == "c2":
                p32 = hs.params(w, 32, 50, seed=5, height=h)
                with ds.progress(cam, p32) as pr:
                    pr.step(16)
                    step16 = pr.step(16)[1].kernel_ms
                row["step16_kernel_ms"] = round(step16, 3)
                row["share_of_1024spp_frame"] = round(gd / (64.0 * step16), 5)
            emit(row)
        finally:
            ds.close()
            hs.close()


def quality_frame(ds, hs, cam, seed, truth_seed, w=256, h=144, spp=16):
    truth = ds.render(cam, hs.params(w, 8192, 50, seed=truth_seed, height=h))[0]
    p = hs.params(w, spp, 50, seed=seed, height=h)
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(4):
            img, _ = pr.step(spp // 4)
        se = pr.stderr()
    color = img.copy()
    old, _ = ds.render_aov(cam, p)
    new, _ = ds.render_guides(cam, p)
    dn_old = ds.denoise(color, se, old["albedo"], old["normal"], old["depth"])[0]
    dn_new = ds.denoise(color, se, new["albedo"], new["normal"], new["depth"])[0]
    delta = new["bounces"] >= 0.5
    return {"noisy": rel_mse(color, truth), "old": rel_mse(dn_old, truth), "new": rel_mse(dn_new, truth),
            "noisy_delta": rel_mse(color, truth, delta), "old_delta": rel_mse(dn_old, truth, delta),
            "new_delta": rel_mse(dn_new, truth, delta), "old_rest": rel_mse(dn_old, truth, ~delta), "new_rest": rel_mse(dn_new, truth, ~delta),
            "delta_share": float(delta.mean()), "mean_bounces": float(new["bounces"].mean())}


def quality_part(args, emit):
    hs = HostScene("random_spheres_iow", 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    frame_ratios = []
    try:
        for seed, truth_seed in SEED_SETS:
            q = quality_frame(ds, hs, cam, seed, truth_seed)
            row = {"part": "quality", "seed": seed, "truth_seed": truth_seed}
            row.update({k: round(v, 6) for k, v in q.items()})
            row["ratio_delta"] = round(q["new_delta"] / q["old_delta"], 4)
            row["ratio_frame"] = round(q["new"] / q["old"], 4)
            row["ratio_rest"] = round(q["new_rest"] / q["old_rest"], 4)
            frame_ratios.append(q["new"] / q["old"])
            emit(row)
        emit({"part": "quality_spread", "ratio_frame_min": round(min(frame_ratios), 4), "ratio_frame_max": round(max(frame_ratios), 4),
              "spread": round(max(frame_ratios) - min(frame_ratios), 4)})
    finally:
        ds.close()
        hs.close()


def temporal_part(args, emit):
    w, h, nframes, spp = 256, 144, 8, 8
    hs = HostScene("random_spheres_demo", 1)
    ds = DeviceScene(hs.desc)
    try:
        cams = [hs.next_camera() for _ in range(nframes)]
        frames = []
        for i, cam in enumerate(cams):
            p = hs.params(w, spp, 50, seed=5 + i, height=h)
            with ds.progress(cam, p, stderr=True) as pr:
                for _ in range(2):
                    img, _ = pr.step(spp // 2)
                se = pr.stderr()
            frames.append({"color": img.copy(), "stderr": se, "first_hit": ds.render_aov(cam, p)[0], "specular": ds.render_guides(cam, p)[0]})
        truth = ds.render(cams[-1], hs.params(w, 8192, 50, seed=77, height=h))[0]
        last = frames[-1]
        delta = last["specular"]["bounces"] >= 0.5
        for kind in ("first_hit", "specular"):
            g = last[kind]
            alone = ds.denoise(last["color"], last["stderr"], g["albedo"], g["normal"], g["depth"])[0]
            shares = []
            with ds.temporal(w, h) as t:
                for cam, f in zip(cams, frames):
                    color, se, hist, _ = t.accumulate(cam, color=f["color"], stderr=f["stderr"], albedo=f[kind]["albedo"],
                                                      normal=f[kind]["normal"], depth=f[kind]["depth"], want_history=True)
                    shares.append(round(t.info().pixels_with_history / (w * h), 4))
            both = ds.denoise(color, se, g["albedo"], g["normal"], g["depth"])[0]
            row = {"part": "temporal", "guides": kind, "scene": "random_spheres_demo", "width": w, "height": h, "frames": nframes, "spp": spp,
                   "delta_share": round(float(delta.mean()), 4), "mean_bounces": round(float(last["specular"]["bounces"].mean()), 4),
                   "history_share_per_frame": shares, "history_share_frame_8_delta": round(float((hist[delta] > 1.0).mean()), 4),
                   "history_share_frame_8_rest": round(float((hist[~delta] > 1.0).mean()), 4)}
            for label, img in (("noisy", last["color"]), ("denoised_alone", alone), ("accumulated", color), ("accumulated_denoised", both)):
                row["relmse_" + label] = round(rel_mse(img, truth), 6)
                row["relmse_" + label + "_delta"] = round(rel_mse(img, truth, delta), 6)
            emit(row)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="time,quality,temporal")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for part in args.part.split(","):
        {"time": time_part, "quality": quality_part, "temporal": temporal_part}[part](args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
