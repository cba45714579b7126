"""Robust film (vk_robust_*): the bucketed deposit and the trimmed resolve on whole frames of camera paths, next to the film's deposit of
the same kind of batch and to device copies of the bytes each touches; and what the estimators buy on cornell_box.  Writes
profiles/robust/report.jsonl (one JSON line per row) and prints them.

    python tools/robust_report.py [--repeats 3] [--cases c2,cornell,final] [--seeds 5] [--out profiles/robust/report.jsonl]

Timing rows.  Frames: those of tools/film_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 —, the scene's own
integrator and background, max_depth 8 (a deposit's work does not depend on how long the paths were).  A window is the frame's bottom
rows, as many as a batch of 2^24 paths holds, at 8 samples per pixel (n_samples <= K for K = 8 and 16: no two lanes share a cell) and at
32 (n_samples > K: 2 to 8 lanes of a wave share a cell).  A batch goes into a robust accumulator once per emit, so every measurement has
a finished batch of its own: emit, step to the end, deposit.  Behind a warm-up round, --repeats rounds run interleaved — per round K = 4,
8, 16 and once the film's deposit —; every value is kept and the median reported.  Times are device milliseconds between two events
around the kernel (vk_debug_robust_last_ms, vk_debug_film_last_ms).  read_copy_ms: a device copy of the 36 bytes per path a deposit
reads.  The resolve of the last state per mode, next to a device copy of the state's bytes (width * height * K * 32) and with the bytes
per second it achieves (state read + the two images written).

Quality rows.  cornell_box 300x300 at 64 samples per pixel, K = 8, against vk_render at 8192 samples per pixel with another seed, for
--seeds seeds: the relative MSE mean((x - t)^2 / (t^2 + 0.01)) of MEAN, GINI and TRIM at tmax over the frame and over the 1 % of the
pixels where MEAN is worst, and of vk_denoise fed each image with its own stderr3.
Nothing passes or fails.  Each case is a timed step of its own: a child process under a time limit; after one fails no further one is
started."""
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
MAX_DEPTH = 8
CAPACITY = 1 << 24
BUCKETS = (4, 8, 16)
med = statistics.median
MODES = (("mean", 0, 0), ("trim_tmax", 1, 0xFFFFFFFF), ("gini", 2, 0))


def r4(xs):
    return [round(float(x), 4) for x in xs]


def timing(key, repeats):
    from film_report import setup
    torch, name, w, h, hs, cam, ds = setup(key)
    from shade_report import copy_ms
    try:
        for ns in (8, 32):
            rows = min(h, CAPACITY // (w * ns))
            n = w * rows * ns
            q = hs.params(w, ns, MAX_DEPTH, seed=2, height=h)
            pb = ds.paths(n)
            film = ds.film(cam, q)
            accs = {K: ds.robust(w, h, ns, buckets=K) for K in BUCKETS}

            def finished_batch():
                film.emit(pb, 0, 0, w, rows, 0, ns)
                pb.step(1 << 20)

            ms = {K: [] for K in BUCKETS}
            film_ms, info = [], {}
            for rep in range(repeats + 1):                              # the first round is the warm-up
                for K in BUCKETS:
                    accs[K].reset()
                    finished_batch()
                    accs[K].deposit(pb)
                    if rep:
                        ms[K].append(accs[K].last_ms()[0])
                    else:
                        info[K] = accs[K].info()
                film.reset()
                film.deposit(pb)                                        # the last finished batch of the round
                if rep:
                    film_ms.append(film.last_ms()[1])
            copies = r4(copy_ms(torch, 36 * n, repeats))
            for K in BUCKETS:
                inf = info[K]
                line = {"part": "deposit", "case": key, "scene": name, "width": w, "height": h, "window_rows": rows, "n_samples": ns, "paths": n,
                        "max_depth": MAX_DEPTH, "buckets": K, "lanes_per_cell": max(1, ns // K), "repeats": repeats,
                        "deposit_ms": round(med(ms[K]), 4), "deposit_ms_all": r4(ms[K]),
                        "film_deposit_ms": round(med(film_ms), 4), "film_deposit_ms_all": r4(film_ms),
                        "over_film": round(med(ms[K]) / med(film_ms), 4),
                        "read_bytes": 36 * n, "read_copy_ms": round(med(copies), 4), "read_copy_ms_all": copies,
                        "deposited": int(inf.deposited), "dropped": int(inf.dropped), "clamped": int(inf.clamped),
                        "atomic_gbytes_per_s": round((int(inf.deposited) * 32 + int(inf.dropped) * 8) / (med(ms[K]) * 1e-3) / 1e9, 2)}
                print(json.dumps(line), flush=True)
            if ns == 8:
                for K in BUCKETS:
                    state_bytes = w * h * K * 32
                    state_copy = r4(copy_ms(torch, 2 * state_bytes, repeats))       # (copy_ms moves nbytes in all: the state read AND written)
                    for label, mode, trim in MODES:
                        got = []
                        for rep in range(repeats + 1):
                            accs[K].resolve(mode=mode, trim=trim, want_stderr=True)
                            if rep:
                                got.append(accs[K].last_ms()[1])
                        moved = state_bytes + 2 * w * h * 12
                        print(json.dumps({"part": "resolve", "case": key, "scene": name, "width": w, "height": h, "buckets": K, "mode": label,
                                          "repeats": repeats, "resolve_ms": round(med(got), 4), "resolve_ms_all": r4(got),
                                          "state_bytes": state_bytes, "state_copy_ms": round(med(state_copy), 4), "state_copy_ms_all": state_copy,
                                          "resolve_gbytes_per_s": round(moved / (med(got) * 1e-3) / 1e9, 1),
                                          "copy_gbytes_per_s": round(2 * state_bytes / (med(state_copy) * 1e-3) / 1e9, 1)}), flush=True)
            for a in accs.values():
                a.close()
            film.close(); pb.close()
    finally:
        ds.close()
        hs.close()


def rel_err(img, truth):
    return ((img.astype(np.float64) - truth) ** 2 / (truth.astype(np.float64) ** 2 + 1e-2)).mean(axis=2)


def quality(seeds):
    import torch            # first: its wheel carries its own HIP runtime, which must be the one that initialises the device
    torch.cuda.init()
    from vecchio_amd import DeviceScene, HostScene
    hs = HostScene("cornell_box", 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    w = h = 300
    spp, K = 64, 8
    try:
        truth = ds.render(cam, hs.params(w, 8192, 50, seed=77, height=h))[0]
        per = {f"{label}{suffix}": [] for label, _, _ in MODES for suffix in ("", "_worst", "_denoised", "_denoised_worst")}
        trimmed = []
        for seed in range(1, seeds + 1):
            q = hs.params(w, spp, 50, seed=seed, height=h)
            with ds.film(cam, q) as film, ds.robust(w, h, spp, buckets=K) as acc, ds.paths(w * h * spp) as pb:
                acc.render(film, pb)
                imgs = {label: acc.resolve(mode=mode, trim=trim, want_stderr=True) for label, mode, trim in MODES}
            worst = None
            for label, _, _ in MODES:
                img, se = imgs[label]
                e = rel_err(img, truth)
                if worst is None:                                       # MODES[0] is MEAN
                    worst = e >= np.quantile(e, 0.99)
                d = rel_err(ds.denoise(img, stderr=se)[0], truth)
                per[label].append(e.mean()); per[f"{label}_worst"].append(e[worst].mean())
                per[f"{label}_denoised"].append(d.mean()); per[f"{label}_denoised_worst"].append(d[worst].mean())
            trimmed.append(float((np.abs(imgs["gini"][0] - imgs["mean"][0]).max(axis=2) > 0).mean()))
        line = {"part": "quality", "scene": "cornell_box", "width": w, "height": h, "samples_per_pixel": spp, "buckets": K, "seeds": seeds,
                "reference_spp": 8192, "gini_differs_from_mean_in_share_of_pixels": round(med(trimmed), 4)}
        for k, v in per.items():
            line[f"relmse_{k}"] = round(med(v), 6)
            line[f"relmse_{k}_all"] = [round(float(x), 6) for x in v]
        print(json.dumps(line), flush=True)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one step and print its lines: a case's key, or `quality`")
    args = ap.parse_args()
    if args.child:
        if args.child == "quality":
            quality(args.seeds)
        else:
            timing(args.child, args.repeats)
        return 0
    lines = []
    status = 0
    for step in [k for k in args.cases.split(",") if k] + (["quality"] if args.seeds else []):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--repeats", str(args.repeats), "--seeds",
                                str(args.seeds)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
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
