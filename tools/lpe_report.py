"""Light-path layers (vk_lpe_*): what the tag of every path costs per bounce and per frame, next to the same frame on vk_paths_step, and the
layered deposit and resolve next to the film's and the robust film's.  Writes profiles/lpe/report.jsonl (one JSON line per row), the
standard layers of the Cornell box as profiles/lpe/cornell_<layer>.pfm, and prints the rows.

    python tools/lpe_report.py [--repeats 3] [--cases c2,cornell,final] [--out profiles/lpe/report.jsonl] [--pfm-dir DIR]

Frames: those of tools/film_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 — at 8 samples per pixel, the
scene's own integrator and background, max_depth 50, one window (the whole frame fits a batch of 2^24 paths), standard_rules().  Behind a
warm-up round, --repeats rounds run interleaved, each: (a) the frame as Film.render walks it, on vk_paths_step, a bounce a call; (b) the
same frame as LightPathLayers.render walks it, on vk_lpe_step, with the layered deposit; then, on (b)'s finished batch, the film's
deposit, the robust film's (K = 8) and the layered one's kernel times.  Wall seconds are the host's, kernel milliseconds the sums of
the steps' kernel_ms (events around each bounce's launches; vk_lpe_step's includes its sixth launch) plus the deposit.  A third pass per
round steps the frame a bounce a call and reads lpe_record_kernel's own time after each (vk_debug_lpe_last_ms), next to a device copy of
the bytes it moves — 36 read per live path (16 of the record, 16 of the hit, the id), 8 of the tag read from the second bounce on, 8
written.  Resolve: every layer and VK_LPE_ALL, kernel time.  Every value is kept and the median reported.  Nothing passes or fails.
Each case is a timed step of its own: a child process under a time limit; after one fails no further one is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = 420
SPP = 8
MAX_DEPTH = 50
med = statistics.median


def r4(xs):
    return [round(float(x), 4) for x in xs]


def frame(key, repeats, out_dir):
    from film_report import setup
    torch, name, w, h, hs, cam, ds = setup(key)
    from shade_report import copy_ms
    from splat_report import write_pfm
    from vecchio_amd import ffi
    from vecchio_amd.scene import STANDARD_LAYERS
    try:
        n = w * h * SPP
        q = hs.params(w, SPP, MAX_DEPTH, seed=2, height=h)
        pb = ds.paths(n)
        film = ds.film(cam, q)
        acc = ds.lpe(w, h, SPP, n)
        rb = ds.robust(w, h, SPP, buckets=8)
        win = (0, 0, w, h, 0, SPP)

        def plain():
            film.reset()
            t0 = time.perf_counter()
            film.emit(pb, *win)
            ms, bounces = 0.0, 0
            while True:
                info = pb.step(1)
                ms += info.kernel_ms
                bounces += info.bounces
                if not info.live:
                    break
            film.deposit(pb)
            img = film.resolve()
            return time.perf_counter() - t0, ms + film.last_ms()[1], bounces, img

        def layered():
            film.reset(); acc.reset(); rb.reset()
            t0 = time.perf_counter()
            film.emit(pb, *win)
            ms = 0.0
            while True:
                info = acc.step(pb, 1)
                ms += info.kernel_ms
                if not info.live:
                    break
            film.deposit(pb)
            acc.deposit(pb)
            img = acc.resolve()
            wall = time.perf_counter() - t0
            rb.deposit(pb)
            return wall, ms + film.last_ms()[1] + acc.last_ms()[1], img

        def per_bounce():
            film.emit(pb, *win)
            rows = []
            while True:
                info = acc.step(pb, 1)
                rows.append((int(info.traced), acc.last_ms()[0], info.kernel_ms))
                if not info.live:
                    break
            return rows

        a_wall, a_ms, b_wall, b_ms, dep = [], [], [], [], {"layers": [], "film": [], "robust8": []}
        bounce_rows = []
        same = True
        for rep in range(repeats + 1):                                  # the first round is the warm-up
            wa, ma, bounces, img_a = plain()
            wb, mb, img_b = layered()
            same = same and img_a.tobytes() == img_b.tobytes()
            rows = per_bounce()
            if rep:
                a_wall.append(wa); a_ms.append(ma); b_wall.append(wb); b_ms.append(mb)
                dep["layers"].append(acc.last_ms()[1]); dep["film"].append(film.last_ms()[1]); dep["robust8"].append(rb.last_ms()[0])
                bounce_rows.append(rows)
        inf = acc.info()
        print(json.dumps({"part": "frame", "case": key, "scene": name, "width": w, "height": h, "samples_per_pixel": SPP, "paths": n,
                          "max_depth": MAX_DEPTH, "bounces": bounces, "repeats": repeats, "all_layers_equal_film_bitwise": same,
                          "paths_step_wall_s": round(med(a_wall), 5), "paths_step_wall_s_all": [round(x, 5) for x in a_wall],
                          "lpe_wall_s": round(med(b_wall), 5), "lpe_wall_s_all": [round(x, 5) for x in b_wall],
                          "wall_ratio": round(med(b_wall) / med(a_wall), 4),
                          "paths_step_kernel_ms": round(med(a_ms), 4), "paths_step_kernel_ms_all": r4(a_ms),
                          "lpe_kernel_ms": round(med(b_ms), 4), "lpe_kernel_ms_all": r4(b_ms), "kernel_ratio": round(med(b_ms) / med(a_ms), 4),
                          "deposited": int(inf.deposited), "dropped": int(inf.dropped), "clamped": int(inf.clamped)}), flush=True)
        print(json.dumps({"part": "deposit", "case": key, "scene": name, "paths": n, "layers": len(STANDARD_LAYERS), "rules": int(inf.n_rules),
                          "repeats": repeats, "layers_deposit_ms": round(med(dep["layers"]), 4), "layers_deposit_ms_all": r4(dep["layers"]),
                          "film_deposit_ms": round(med(dep["film"]), 4), "film_deposit_ms_all": r4(dep["film"]),
                          "robust8_deposit_ms": round(med(dep["robust8"]), 4), "robust8_deposit_ms_all": r4(dep["robust8"]),
                          "over_film": round(med(dep["layers"]) / med(dep["film"]), 4),
                          "over_robust8": round(med(dep["layers"]) / med(dep["robust8"]), 4)}), flush=True)
        for b in range(min(len(r) for r in bounce_rows)):
            live = bounce_rows[0][b][0]
            moved = live * (52 if b else 44)
            rec = [r[b][1] for r in bounce_rows]
            whole = [r[b][2] for r in bounce_rows]
            copies = r4(copy_ms(torch, moved, repeats))
            if b < 8 or b % 8 == 0:
                print(json.dumps({"part": "record", "case": key, "scene": name, "bounce": b, "live": live, "bytes_moved": moved,
                                  "record_ms": round(med(rec), 4), "record_ms_all": r4(rec), "copy_ms": round(med(copies), 4), "copy_ms_all": copies,
                                  "bounce_kernel_ms": round(med(whole), 4), "share_of_bounce": round(med(rec) / med(whole), 4),
                                  "record_gbytes_per_s": round(moved / (med(rec) * 1e-3) / 1e9, 1)}), flush=True)
        total_rec = [sum(x[1] for x in r) for r in bounce_rows]
        total_all = [sum(x[2] for x in r) for r in bounce_rows]
        print(json.dumps({"part": "record_total", "case": key, "scene": name, "record_ms": round(med(total_rec), 4), "record_ms_all": r4(total_rec),
                          "bounces_kernel_ms": round(med(total_all), 4), "share": round(med(total_rec) / med(total_all), 4)}), flush=True)
        for layer in list(range(len(STANDARD_LAYERS))) + [ffi.VK_LPE_ALL]:
            got = []
            for rep in range(repeats + 1):
                img, share = acc.resolve(layer, want_share=True)
                if rep:
                    got.append(acc.last_ms()[2])
            label = "all" if layer == ffi.VK_LPE_ALL else STANDARD_LAYERS[layer]
            print(json.dumps({"part": "resolve", "case": key, "scene": name, "layer": label, "resolve_ms": round(med(got), 4), "resolve_ms_all": r4(got),
                              "mean_share": round(float(share.mean()), 5), "mean_rgb": r4(img.reshape(-1, 3).mean(axis=0))}), flush=True)
            if key == "cornell" and layer != ffi.VK_LPE_ALL:
                os.makedirs(out_dir, exist_ok=True)
                write_pfm(os.path.join(out_dir, f"cornell_{label}.pfm"), img)
        rb.close(); acc.close(); film.close(); pb.close()
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpe", "report.jsonl"))
    ap.add_argument("--pfm-dir", default=None, help="where the Cornell box's layers go (default: next to the report)")
    ap.add_argument("--child", default=None, help="(internal) run one case and print its lines")
    args = ap.parse_args()
    out_dir = os.path.abspath(args.pfm_dir) if args.pfm_dir else os.path.dirname(os.path.abspath(args.out))
    if args.child:
        frame(args.child, args.repeats, out_dir)
        return 0
    lines = []
    status = 0
    for step in [k for k in args.cases.split(",") if k]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--repeats", str(args.repeats), "--out", args.out, "--pfm-dir", out_dir],
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
