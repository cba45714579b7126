"""Display transform (vk_tone_*): the meter kernel in both forms and the encode kernel's instances on whole frames, next to
vk_to_color_device on the same frame and to device copies of the bytes each touches.  Writes profiles/tone/report.jsonl (one JSON line per
row) and prints them.

    python tools/tone_report.py [--repeats 9] [--cases c2,cornell,final] [--out profiles/tone/report.jsonl]

Frames: those of tools/film_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 — rendered once at 8 samples per
pixel, max_depth 8; beside the rendered frame a flat frame (every pixel 0.18: the meter's contention case) and log-uniform noise over 30
octaves.  Behind a warm-up round, --repeats rounds run interleaved — per round and content the meter's LDS form, its plain form, then
the encode's reference instance (CLAMP), ACES + sRGB, ACES + sRGB + dither, and vk_to_color_device —; every value is kept, the median
and the spread (min, max) reported.  Times are device milliseconds between two events around the kernel (vk_debug_tone_last_ms; torch
events around vk_to_color_device).  Copies: a device-to-device copy that reads the frame's bytes and writes as many (next to the meter,
which only reads them), and one that moves what an encode reads and writes (12 + 3 bytes a pixel).  Bytes per second are the bytes a
kernel must move — the meter 12 a pixel, an encode 15 — over its median time.  Nothing passes or fails.  Each case is a timed step of
its own: a child process under a time limit; after one fails no further one is started."""
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

STEP_LIMIT_S = 300
med = statistics.median


def r4(xs):
    return [round(float(x), 4) for x in xs]


def spread(xs):
    return {"median": round(med(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def timing(key, repeats):
    from film_report import setup
    torch, name, w, h, hs, cam, ds = setup(key)
    from shade_report import copy_ms
    from vecchio_amd import ffi
    try:
        n = w * h
        rendered, _ = ds.render(cam, hs.params(w, 8, 8, seed=2, height=h))
        rng = np.random.default_rng(1)
        frames = {"rendered": rendered, "flat": np.full((h, w, 3), 0.18, np.float32),
                  "noise": np.exp2(rng.uniform(-15, 15, (h, w, 3))).astype(np.float32)}
        forms = (("lds", ffi.VK_TONE_FORM_LDS), ("plain", ffi.VK_TONE_FORM_PLAIN))
        encodes = (("reference", dict(curve=ffi.VK_TONE_CLAMP, transfer=ffi.VK_TONE_TRANSFER_REFERENCE, flags=0)),
                   ("aces_srgb", dict(curve=ffi.VK_TONE_ACES, transfer=ffi.VK_TONE_TRANSFER_SRGB, flags=ffi.VK_TONE_USE_METERED)),
                   ("aces_srgb_dither", dict(curve=ffi.VK_TONE_ACES, transfer=ffi.VK_TONE_TRANSFER_SRGB,
                                             flags=ffi.VK_TONE_USE_METERED | ffi.VK_TONE_DITHER)))
        tone = ds.tone(w, h)
        d_out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        meter_ms = {(c, f): [] for c in frames for f, _ in forms}
        encode_ms = {(c, e): [] for c in frames for e, _ in encodes}
        to_color_ms = {c: [] for c in frames}
        d_frames = {c: torch.from_numpy(a).cuda() for c, a in frames.items()}
        for rep in range(repeats + 1):                                   # the first round is the warm-up
            for c in frames:
                tone.load_device(d_frames[c])
                for f, form in forms:
                    tone.set_form(form)
                    tone.meter()
                    if rep:
                        meter_ms[c, f].append(tone.last_ms()[0])
                for e, kw in encodes:
                    tone.encode_device(d_out, **kw)
                    if rep:
                        encode_ms[c, e].append(tone.last_ms()[1])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ds.to_color_device(d_frames[c].data_ptr(), w, h, d_out.data_ptr())
                e1.record()
                e1.synchronize()
                if rep:
                    to_color_ms[c].append(e0.elapsed_time(e1))
        read_copy = copy_ms(torch, 2 * 12 * n, repeats)                  # (copy_ms moves nbytes in all: the frame read AND written)
        moved_copy = copy_ms(torch, 15 * n, repeats)
        base = {"case": key, "scene": name, "width": w, "height": h, "pixels": n, "repeats": repeats}
        for c in frames:
            line = dict(base, part="meter", content=c, frame_bytes=12 * n, frame_copy_ms=spread(read_copy),
                        frame_copy_gbytes_per_s=round(2 * 12 * n / (med(read_copy) * 1e-3) / 1e9, 1))
            for f, _ in forms:
                line[f"{f}_ms"] = spread(meter_ms[c, f])
                line[f"{f}_ms_all"] = r4(meter_ms[c, f])
                line[f"{f}_gbytes_per_s"] = round(12 * n / (med(meter_ms[c, f]) * 1e-3) / 1e9, 1)
            line["lds_over_plain"] = round(med(meter_ms[c, "lds"]) / med(meter_ms[c, "plain"]), 4)
            print(json.dumps(line), flush=True)
            line = dict(base, part="encode", content=c, moved_bytes=15 * n, moved_copy_ms=spread(moved_copy),
                        moved_copy_gbytes_per_s=round(15 * n / (med(moved_copy) * 1e-3) / 1e9, 1),
                        to_color_ms=spread(to_color_ms[c]), to_color_ms_all=r4(to_color_ms[c]),
                        to_color_gbytes_per_s=round(15 * n / (med(to_color_ms[c]) * 1e-3) / 1e9, 1))
            for e, _ in encodes:
                line[f"{e}_ms"] = spread(encode_ms[c, e])
                line[f"{e}_ms_all"] = r4(encode_ms[c, e])
                line[f"{e}_gbytes_per_s"] = round(15 * n / (med(encode_ms[c, e]) * 1e-3) / 1e9, 1)
            line["reference_over_to_color"] = round(med(encode_ms[c, "reference"]) / med(to_color_ms[c]), 4)
            print(json.dumps(line), flush=True)
        tone.close()
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tone", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its lines")
    args = ap.parse_args()
    if args.child:
        timing(args.child, args.repeats)
        return 0
    lines = []
    status = 0
    for step in [k for k in args.cases.split(",") if k]:
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
