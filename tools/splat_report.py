"""Reconstruction filters (vk_splat_*): the deposit kernel's two forms, PLAIN and TILED, on whole frames of camera paths, next to the
film's box deposit of the same kind of batch and to a device copy of the bytes a deposit reads.  Writes profiles/splat/report.jsonl
(one JSON line per row, then one summary line) and prints them.

    python tools/splat_report.py [--repeats 3] [--cases c2,cornell,final] [--spp 1,8] [--out profiles/splat/report.jsonl]

Frames: those of tools/film_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 — at 1 and at 8 samples per pixel,
one emit of all of them, the scene's own integrator and background, max_depth 8 (a deposit's work does not depend on how long the paths
were; the short depth keeps the tracing between two deposits short).  Filters: BOX at 0.5, TENT at 1, MITCHELL at 2 (1/3, 1/3): 18 rows.

A batch goes into an accumulator once per emit, so every measurement has a finished batch of its own: emit, step to the end, deposit.
Behind a warm-up round, --repeats rounds run interleaved — per round, for each filter, PLAIN then TILED, and once the film's deposit —;
every value is kept, the median and the spread are reported.  Times are device milliseconds between two events around the kernel
(vk_debug_splat_last_ms, vk_debug_film_last_ms).  plain_atomic_gbytes_per_s: contributions x 4 sums x 8 bytes over PLAIN's time.
The form that is faster (by the medians) on the majority of the rows is the summary line's `default_form`.  At 8 samples per pixel a crop
of C2's frame is written as profiles/splat/c2_crop_box.pfm and c2_crop_mitchell.pfm (not kept in the repository).
Nothing passes or fails.  Each (frame, samples) pair is a timed step of its own: a child process under a time limit; after one fails no
further one is started."""
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
CROP = (800, 380, 320, 240)            # x0, y0 (from the bottom), width, height: sphere silhouettes of C2's frame
f32 = np.float32
med = statistics.median
FILTERS = [("box0.5", 0, 0.5), ("tent1", 1, 1.0), ("mitchell2", 2, 2.0)]


def r4(xs):
    return [round(float(x), 4) for x in xs]


def write_pfm(path, img):
    """img (h, w, 3) float32, row 0 the bottom row (PFM's own order)"""
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(img, "<f4").tobytes())


def frame(key, spp, repeats, out_dir):
    from film_report import setup
    torch, name, w, h, hs, cam, ds = setup(key)
    from shade_report import copy_ms
    from vecchio_amd import ffi
    try:
        n = w * h * spp
        q = hs.params(w, spp, MAX_DEPTH, seed=2, height=h)
        pb = ds.paths(n)
        film = ds.film(cam, q)
        accs = {label: ds.splat(w, h, spp, filter=kind, radius=radius) for label, kind, radius in FILTERS}

        def finished_batch():
            film.emit(pb, 0, 0, w, h, 0, spp)
            pb.step(1 << 20)

        ms = {(label, form): [] for label, _, _ in FILTERS for form in (1, 2)}
        film_ms, same, info = [], {}, {}
        for rep in range(repeats + 1):                              # the first round is the warm-up
            for label, _, _ in FILTERS:
                acc = accs[label]
                sums = {}
                for form in (ffi.VK_DEBUG_SPLAT_FORM_PLAIN, ffi.VK_DEBUG_SPLAT_FORM_TILED):
                    acc.reset()
                    acc.debug_form(form)
                    finished_batch()
                    acc.deposit(pb)
                    if rep:
                        ms[(label, form)].append(acc.last_ms()[0])
                    else:
                        sums[form] = acc.debug_sums().tobytes()
                        info[label] = acc.info()
                if not rep:
                    same[label] = sums[1] == sums[2]
            film.reset()
            film.deposit(pb)                                        # the last finished batch of the round
            if rep:
                film_ms.append(film.last_ms()[1])
        copies = r4(copy_ms(torch, 36 * n, repeats))
        for label, kind, radius in FILTERS:
            plain, tiled, inf = ms[(label, 1)], ms[(label, 2)], info[label]
            line = {"case": key, "scene": name, "width": w, "height": h, "samples_per_pixel": spp, "paths": n, "max_depth": MAX_DEPTH,
                    "filter": label, "repeats": repeats,
                    "plain_ms": round(med(plain), 4), "plain_ms_all": r4(plain), "tiled_ms": round(med(tiled), 4), "tiled_ms_all": r4(tiled),
                    "tiled_over_plain": round(med(tiled) / med(plain), 4),
                    "tiled_wins_beyond_the_spread": bool(max(tiled) < min(plain)), "plain_wins_beyond_the_spread": bool(max(plain) < min(tiled)),
                    "film_deposit_ms": round(med(film_ms), 4), "film_deposit_ms_all": r4(film_ms),
                    "read_bytes": 36 * n, "read_copy_ms": round(med(copies), 4), "read_copy_ms_all": copies,
                    "contributions": int(inf.contributions), "deposited": int(inf.deposited), "dropped": int(inf.dropped),
                    "clamped": int(inf.clamped),
                    "plain_atomic_gbytes_per_s": round(int(inf.contributions) * 32 / (med(plain) * 1e-3) / 1e9, 2),
                    "same_bytes": bool(same[label])}
            print(json.dumps(line), flush=True)
        if key == "c2" and spp == 8:
            x0, y0, cw, ch = CROP
            os.makedirs(out_dir, exist_ok=True)
            for label, tag in (("box0.5", "box"), ("mitchell2", "mitchell")):
                write_pfm(os.path.join(out_dir, f"c2_crop_{tag}.pfm"), accs[label].resolve()[y0:y0 + ch, x0:x0 + cw])
        for a in accs.values():
            a.close()
        film.close(); pb.close()
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--spp", default="1,8")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splat", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one (frame, samples) pair and print its lines: KEY:SPP")
    args = ap.parse_args()
    out_dir = os.path.dirname(os.path.abspath(args.out))
    if args.child:
        key, spp = args.child.split(":")
        frame(key, int(spp), args.repeats, out_dir)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        for spp in args.spp.split(","):
            if status:
                break
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{key}:{spp}", "--repeats", str(args.repeats),
                                    "--out", args.out], capture_output=True, text=True, timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f"case {key}:{spp} ran into its time limit of {STEP_LIMIT_S} s; nothing further is started", file=sys.stderr)
                status = 1
                break
            got = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
            lines += got
            print("\n".join(got), flush=True)
            if r.returncode != 0:
                print(f"case {key}:{spp} ended with status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", file=sys.stderr)
                status = 1
    rows = [json.loads(ln) for ln in lines]
    if rows:
        tiled = sum(r["tiled_ms"] < r["plain_ms"] for r in rows)
        lines.append(json.dumps({"summary": True, "rows": len(rows), "tiled_faster_on": tiled, "plain_faster_or_level_on": len(rows) - tiled,
                                 "default_form": "TILED" if 2 * tiled > len(rows) else "PLAIN"}))
        print(lines[-1], flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
