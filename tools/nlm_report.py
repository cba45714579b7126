"""Non-local means (vk_nlm_*): the filter kernel in both forms on whole frames next to the default vk_denoise call and one 16-spp
progressive step, and what the filter does to the relative MSE of rendered frames.  Writes profiles/nlm/report.jsonl (one JSON line per
row) and prints them.

    python tools/nlm_report.py [--repeats 7] [--steps c2,cornell,final,quality_cornell,quality_iow] [--out profiles/nlm/report.jsonl]

Timing (steps c2, cornell, final: C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800): the frame is rendered once at 16 samples
per pixel in 4 windows of a progress handle (its stderr() is the filter's variance), albedo, normal and depth come from render_aov.  Behind
a warm-up round, --repeats rounds run interleaved — per round the PLAIN and the TILED form at (R, F) = (3, 1), (7, 3), (10, 3) and at
(1, 0), (10, 0), (7, 2), (1, 1), (2, 2), (1, 3), (10, 1), the default vk_denoise call and one progressive step of 16 samples —; every value is kept, the median and the spread (min, max) reported.
Times are device milliseconds: vk_debug_nlm_last_ms (two events around the filter kernel), vk_denoise's and the step's own kernel_ms.
Quality (steps quality_cornell: cornell_box 256x256, quality_iow: random_spheres_iow 256x144): at 4 / 16 / 64 samples per pixel over
five seeds the relative MSE mean((x - t)^2 / (t^2 + 0.01)) against 8192 spp of another seed, of the noisy frame, vk_denoise, vk_nlm and
vk_nlm followed by vk_denoise (which is handed the filter's stderr3_out), and a sweep of k and of R.  Nothing passes or fails.
Each step is a child process under a time limit; after one fails no further one is started."""
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

STEP_LIMIT_S = 420
# the three report rows, then what AUTO's table needs: no patch at either end of R, and the smallest windows with a patch
RADII = ((3, 1), (7, 3), (10, 3), (1, 0), (10, 0), (7, 2), (1, 1), (2, 2), (1, 3), (10, 1))
QUALITY = {"quality_cornell": ("cornell_box", 256, 256), "quality_iow": ("random_spheres_iow", 256, 144)}
med = statistics.median


def spread(xs):
    return {"median": round(med(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def rel_mse(x, t):
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    return float(np.mean((x - t) ** 2 / (t ** 2 + 0.01)))


def noisy_frame(ds, hs, cam, w, h, spp, seed, windows=4):
    p = hs.params(w, spp, 50, seed=seed, height=h)
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(windows):
            img, _ = pr.step(spp // windows)
        se = pr.stderr()
    aov, _ = ds.render_aov(cam, p)
    return img.copy(), se, aov


def timing(key, repeats):
    from film_report import setup
    torch, name, w, h, hs, cam, ds = setup(key)
    from vecchio_amd import ffi
    try:
        color, se, aov = noisy_frame(ds, hs, cam, w, h, 16, 2)
        forms = (("plain", ffi.VK_NLM_FORM_PLAIN), ("tiled", ffi.VK_NLM_FORM_TILED))
        ms = {(r, f, n): [] for r, f in RADII for n, _ in forms}
        prepare_ms, denoise_ms, step_ms = [], [], []
        d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        d_se = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        p = hs.params(w, 16, 50, seed=2, height=h)
        with ds.nlm(w, h) as nl, ds.progress(cam, p) as pr:
            for rep in range(repeats + 1):                                   # the first round is the warm-up
                nl.load(color, se, aov["albedo"])
                if rep:
                    prepare_ms.append(nl.last_ms()[0])
                for r, f in RADII:
                    for n, form in forms:
                        nl.set_form(form)
                        nl.filter_device(d_out, d_se, search_radius=r, patch_radius=f)
                        if rep:
                            ms[r, f, n].append(nl.last_ms()[1])
                _, st = ds.denoise(color, se, aov["albedo"], aov["normal"], aov["depth"])
                pr.reset()
                _, sp = pr.step(16)
                if rep:
                    denoise_ms.append(st.kernel_ms)
                    step_ms.append(sp.kernel_ms)
        line = {"part": "timing", "case": key, "scene": name, "width": w, "height": h, "repeats": repeats, "prepare_ms": spread(prepare_ms),
                "denoise_default_ms": spread(denoise_ms), "step_16spp_ms": spread(step_ms)}
        for r, f in RADII:
            for n, _ in forms:
                line[f"R{r}F{f}_{n}_ms"] = spread(ms[r, f, n])
                line[f"R{r}F{f}_{n}_ms_all"] = [round(x, 4) for x in ms[r, f, n]]
            line[f"R{r}F{f}_tiled_over_plain"] = round(med(ms[r, f, "tiled"]) / med(ms[r, f, "plain"]), 4)
        print(json.dumps(line), flush=True)
    finally:
        ds.close()
        hs.close()


def quality(key):
    import torch
    torch.cuda.init()
    from vecchio_amd import DeviceScene, HostScene
    name, w, h = QUALITY[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        truth, _ = ds.render(cam, hs.params(w, 8192, 50, seed=4242, height=h))
        base = {"part": "quality", "scene": name, "width": w, "height": h, "reference_spp": 8192}
        with ds.nlm(w, h) as nl:
            for spp in (4, 16, 64):
                rows = {v: [] for v in ("noisy", "denoise", "nlm", "nlm_then_denoise")}
                sweep_k = {k: [] for k in (0.3, 0.45, 0.6, 0.7, 0.85, 1.0)}
                sweep_r = {r: [] for r in (3, 5, 7, 10)}
                for seed in (11, 12, 13, 14, 15):
                    color, se, aov = noisy_frame(ds, hs, cam, w, h, spp, seed)
                    nl.load(color, se, aov["albedo"])
                    out, out_se = nl.filter()
                    dn, _ = ds.denoise(color, se, aov["albedo"], aov["normal"], aov["depth"])
                    both, _ = ds.denoise(out, out_se, aov["albedo"], aov["normal"], aov["depth"])
                    for v, img in (("noisy", color), ("denoise", dn), ("nlm", out), ("nlm_then_denoise", both)):
                        rows[v].append(rel_mse(img, truth))
                    for k in sweep_k:
                        sweep_k[k].append(rel_mse(nl.filter(k=k)[0], truth) / rows["noisy"][-1])
                    for r in sweep_r:
                        sweep_r[r].append(rel_mse(nl.filter(search_radius=r)[0], truth) / rows["noisy"][-1])
                line = dict(base, spp=spp, seeds=5)
                for v, xs in rows.items():
                    line[f"{v}_rel_mse"] = round(float(np.mean(xs)), 6)
                    if v != "noisy":
                        line[f"{v}_ratio"] = round(float(np.mean(xs) / np.mean(rows["noisy"])), 4)
                        line[f"{v}_ratio_per_seed"] = [round(a / b, 4) for a, b in zip(xs, rows["noisy"])]
                line["sweep_k_ratio"] = {str(k): round(float(np.mean(v)), 4) for k, v in sweep_k.items()}
                line["sweep_R_ratio"] = {str(r): round(float(np.mean(v)), 4) for r, v in sweep_r.items()}
                print(json.dumps(line), flush=True)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="c2,cornell,final,quality_cornell,quality_iow")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlm", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one step and print its lines")
    args = ap.parse_args()
    if args.child:
        quality(args.child) if args.child in QUALITY else timing(args.child, args.repeats)
        return 0
    lines = []
    status = 0
    for step in [k for k in args.steps.split(",") if k]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--repeats", str(args.repeats)],
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
