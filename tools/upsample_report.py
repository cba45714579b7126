"""Guided upsampling (vk_upsample_*): one apply in both forms on whole frames next to a device copy of the bytes it must move, and what
render scale buys at equal paths and at a quarter of the paths.  Writes profiles/upsample/report.jsonl (one JSON line per row) and prints
them.

    python tools/upsample_report.py [--repeats 9] [--steps c2,cornell,final,quality_cornell,quality_iow] [--out profiles/upsample/report.jsonl]

Timing (steps c2, cornell, final: C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800), from half and from quarter size: the low
frame (16 samples per pixel in four windows, with its stderr3) and the first-hit buffers of both sizes are rendered once and stay on the
device.  Behind a warm-up round, --repeats rounds run interleaved — per round and ratio the PLAIN and then the TILED form
(vk_upsample_apply_device with every guide and stderr3_out, the library's defaults), then the copy —; every value is kept, the median and
the spread (min, max) reported.  A sample is BATCH = 20 calls back to back between two events on the null stream (the stream every one of
these calls runs on), divided by 20, in device milliseconds: one apply is one kernel of tens of microseconds, too short a window for two
events.  So a figure is what a call costs in a stream of such calls, the counters' memset and launch gaps included.  Before the rounds
each frame's TILED output is compared with its PLAIN output bit for bit; a difference ends the step.

The bytes an apply must move: the high guides in (albedo and normal 12 bytes a pixel, depth 4) and two frames out (12 each): 52 W H; the
low planes (48 w h) are read many times out of caches and not counted: the copy is the floor, not a model.

Quality (steps quality_cornell 256x256, quality_iow 256x144: tools/nlm_report.py's scenes): over five seeds the relative MSE mean((x -
t)^2 / (t^2 + 0.01)) against 8192 spp of another seed, for n = 4 and 16 samples per pixel, of (full) the full-size frame at n; (equal) the
half-size frame at 4 n, upsampled: the same number of paths; (quarter) the half-size frame at n, upsampled: a quarter of the paths; each
plain and through vk_denoise with the library's defaults, the upsampler's sigma_z over 0.5, 1, 2, 4 and normal_squarings over 3, 5, 7.
A lamp that lies in the plane of its ceiling differs from it in neither normal nor depth, so its edge is upsampled by the tent alone: the
rows ending in _away leave out every pixel within 8 pixels of one whose reference is brighter than 4 (cornell_box's lamp; random_spheres_iow
has none), for the full frame and the default parameters.
Nothing passes or fails.  Each step is a child process under a time limit; after one fails no further one is started."""
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

STEP_LIMIT_S = 280
BATCH = 20
RATIOS = (("half", 2), ("quarter", 4))
SIGMAS, SQUARINGS = (0.5, 1.0, 2.0, 4.0), (3, 5, 7)
med = statistics.median


def spread(xs):
    return {"median": round(med(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def batch_ms(torch, call):
    """BATCH calls back to back between two events on the null stream: device milliseconds per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(BATCH):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / BATCH


def timing(key, repeats):
    from film_report import setup
    from nlm_report import noisy_frame
    torch, name, W, H, hs, cam, ds = setup(key)
    from vecchio_amd import ffi
    try:
        assert torch.cuda.current_stream().cuda_stream == 0                  # torch's events are recorded on the null stream
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
        hi, _ = ds.render_aov(cam, hs.params(W, 4, 50, seed=2, height=H), want=("albedo", "normal", "depth"))
        d_hi = [dev(hi[k]) for k in ("albedo", "normal", "depth")]
        d_out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        d_se = torch.zeros_like(d_out)
        nbytes = 52 * W * H
        src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.zeros_like(src)
        forms = (("plain", ffi.VK_UPSAMPLE_FORM_PLAIN), ("tiled", ffi.VK_UPSAMPLE_FORM_TILED))
        handles, ms, copies, counts = {}, {}, [], {}
        for rname, div in RATIOS:
            w, h = W // div, H // div
            color, se, lo = noisy_frame(ds, hs, cam, w, h, 16, 2)
            u = ds.upsample(w, h, W, H)
            u.load_device(dev(color), dev(se), dev(lo["albedo"]), dev(lo["normal"]), dev(lo["depth"]))
            handles[rname] = u
            outs = []
            for n, form in forms:                                             # the two forms give the same bits on this frame
                u.set_form(form)
                u.apply_device(d_out, d_se, *d_hi)
                torch.cuda.synchronize()
                outs.append((d_out.view(torch.int32).clone(), d_se.view(torch.int32).clone()))
                ms[rname, n] = []
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"{key} {rname}: TILED differs from PLAIN"
            counts[rname] = (int(u.info().fallback_pixels), int(u.info().empty_pixels), w, h)
        for rep in range(repeats + 1):                                        # the first round is the warm-up
            for rname, _ in RATIOS:
                u = handles[rname]
                p = u.params()
                for n, form in forms:
                    u.set_form(form)
                    took = batch_ms(torch, lambda: u.apply_device(d_out, d_se, *d_hi, params=p))
                    if rep:
                        ms[rname, n].append(took)
            c = batch_ms(torch, lambda: dst.copy_(src))
            if rep:
                copies.append(c)
        line = {"part": "timing", "case": key, "scene": name, "width": W, "height": H, "repeats": repeats, "batch": BATCH,
                "tiled_equals_plain": True, "bytes": nbytes, "copy_ms": spread(copies)}
        for rname, _ in RATIOS:
            fb, em, w, h = counts[rname]
            line[f"{rname}_low"] = [w, h]
            line[f"{rname}_fallback_pixels"], line[f"{rname}_empty_pixels"] = fb, em
            for n, _ in forms:
                line[f"{rname}_{n}_ms"] = spread(ms[rname, n])
                line[f"{rname}_{n}_ms_all"] = [round(x, 4) for x in ms[rname, n]]
            line[f"{rname}_tiled_over_plain"] = round(med(ms[rname, "tiled"]) / med(ms[rname, "plain"]), 4)
            line[f"{rname}_plain_over_copy"] = round(med(ms[rname, "plain"]) / med(copies), 4)
        for u in handles.values():
            u.close()
        print(json.dumps(line), flush=True)
    finally:
        ds.close()
        hs.close()


def quality(key):
    import torch
    torch.cuda.init()
    from nlm_report import QUALITY, noisy_frame, rel_mse
    from vecchio_amd import DeviceScene, HostScene
    name, W, H = QUALITY[key]
    w, h = W // 2, H // 2
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        truth, _ = ds.render(cam, hs.params(W, 8192, 50, seed=4242, height=H))
        lamp = truth.max(-1) > 4.0
        near = np.zeros_like(lamp)
        for dy in range(-8, 9):
            for dx in range(-8, 9):
                near |= np.roll(np.roll(lamp, dy, 0), dx, 1)
        away = ~near
        base = {"part": "quality", "scene": name, "width": W, "height": H, "low": [w, h], "reference_spp": 8192,
                "pixels_near_a_lamp": int(near.sum())}
        mean = lambda xs: round(float(np.mean(xs)), 6)
        with ds.upsample(w, h, W, H) as u:
            for n in (4, 16):
                rows = {}
                add = lambda k, img: rows.setdefault(k, []).append(rel_mse(img, truth))
                add_away = lambda k, img: rows.setdefault(k + "_away", []).append(rel_mse(img[away], truth[away]))
                fallbacks = []
                for seed in (11, 12, 13, 14, 15):
                    full, full_se, hi = noisy_frame(ds, hs, cam, W, H, n, seed)
                    full_dn = ds.denoise(full, full_se, hi["albedo"], hi["normal"], hi["depth"])[0]
                    for f in (add, add_away):
                        f("full", full)
                        f("full_denoised", full_dn)
                    for tag, spp in (("equal", 4 * n), ("quarter", n)):
                        color, se, lo = noisy_frame(ds, hs, cam, w, h, spp, seed)
                        u.load(color, se, lo["albedo"], lo["normal"], lo["depth"])
                        out, _ = u.apply(hi["albedo"], None, None)
                        add(f"{tag}_albedo_only", out)
                        for sz in SIGMAS:
                            for sq in SQUARINGS:
                                out, out_se = u.apply(hi["albedo"], hi["normal"], hi["depth"], sigma_z=sz, normal_squarings=sq)
                                dn = ds.denoise(out, out_se, hi["albedo"], hi["normal"], hi["depth"])[0]
                                add(f"{tag}_s{sz}_q{sq}", out)
                                add(f"{tag}_s{sz}_q{sq}_denoised", dn)
                                if (sz, sq) == (1.0, 7):
                                    fallbacks.append(int(u.info().fallback_pixels))
                                    add_away(f"{tag}_default", out)
                                    add_away(f"{tag}_default_denoised", dn)
                line = dict(base, spp=n, seeds=5, fallback_pixels_default=fallbacks)
                for k, xs in rows.items():
                    line[k] = mean(xs)
                for tag in ("equal", "quarter"):
                    for sfx in ("", "_denoised"):
                        best = min(((line[f"{tag}_s{sz}_q{sq}{sfx}"], sz, sq) for sz in SIGMAS for sq in SQUARINGS))
                        line[f"{tag}{sfx}_best"] = {"rel_mse": best[0], "sigma_z": best[1], "normal_squarings": best[2]}
                        line[f"{tag}{sfx}_default_over_full"] = round(line[f"{tag}_s1.0_q7{sfx}"] / line["full" + sfx], 4)
                print(json.dumps(line), flush=True)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="c2,cornell,final,quality_cornell,quality_iow")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one step and print its lines")
    args = ap.parse_args()
    out_dir = os.path.dirname(os.path.abspath(args.out))
    if args.child:
        quality(args.child) if args.child.startswith("quality") else timing(args.child, args.repeats)
        return 0
    os.makedirs(out_dir, exist_ok=True)
    lines = []
    status = 0
    for step in [k for k in args.steps.split(",") if k]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--repeats", str(args.repeats), "--out", args.out],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"step {step} ran into its time limit of {STEP_LIMIT_S} s; nothing further is started", file=sys.stderr)
            status = 1
            break
        got = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
        lines += got
        print("\n".join(got), flush=True)
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", file=sys.stderr)
            status = 1
            break
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
