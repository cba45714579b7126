"""Glare (vk_glare_*): one apply in both forms on whole frames next to a device copy of the bytes it must move and to vk_tone_encode_device
on the same frame, and the Cornell box's lamp with and without glare.  Writes profiles/glare/report.jsonl (one JSON line per row) and
prints them.

    python tools/glare_report.py [--repeats 9] [--steps c2,cornell,final,lamp] [--out profiles/glare/report.jsonl]

Timing (steps c2, cornell, final: C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800): the frame is rendered once at 4
samples per pixel and stays on the device.  Behind a warm-up round, --repeats rounds run interleaved — per round, for L = 4, 6 and 8, the
PLAIN and then the FUSED form (vk_glare_apply_device, the library's other defaults), then the copy, then the encode —; every value is
kept, the median and the spread (min, max) reported.  A sample is BATCH = 20 calls back to back between two events on the null stream
(the stream every one of these calls runs on), divided by 20, in device milliseconds: one apply is tens of microseconds and up to 14
launches, too short a window for two events.  So a figure is what a call costs in a stream of such calls, launch gaps included.
Before the rounds each frame's FUSED output is compared with its PLAIN output bit for bit at every L; a difference ends the step.

The bytes an apply must move, with F = width * height * 12 and P_l = w_l * h_l * 12: the frame is read twice (by the first down pass and
by the composite) and written once, 3 F; every B_l, l = 1 .. L - 1, is written once and read once on the way up, and all but the last are
read once more by the next down pass; every A_l, l = 1 .. L - 2, is written once and read once.  What a form reads again out of caches
(halos, the taps of neighbouring pixels) is not counted: the copy is the floor, not a model.

Step lamp: cornell_box at 900x900 and 64 samples per pixel through ACES and sRGB at the metered exposure of the frame without glare,
without and with glare at the library's defaults; a 240 x 160 crop around the brightest pixel of each goes to lamp_plain.ppm and
lamp_glare.ppm beside the report.  Nothing passes or fails.  Each step is a child process under a time limit; after one fails no
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

STEP_LIMIT_S = 240
BATCH = 20
LEVELS = (4, 6, 8)
med = statistics.median


def spread(xs):
    return {"median": round(med(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def bytes_moved(w, h, L):
    sizes = [(w, h)]
    for _ in range(1, L):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    P = [a * b * 12 for a, b in sizes]
    total = 3 * P[0]
    for l in range(1, L):
        total += P[l] * (3 if l < L - 1 else 2)
    for l in range(1, L - 1):
        total += P[l] * 2
    return total


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
    torch, name, w, h, hs, cam, ds = setup(key)
    from vecchio_amd import ffi
    try:
        frame, _ = ds.render(cam, hs.params(w, 4, 50, seed=2, height=h))
        d_in = torch.from_numpy(np.ascontiguousarray(frame, np.float32).reshape(h, w, 3)).cuda()
        d_out = torch.zeros_like(d_in)
        d_codes = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        forms = (("plain", ffi.VK_GLARE_FORM_PLAIN), ("fused", ffi.VK_GLARE_FORM_FUSED))
        ms = {(L, n): [] for L in LEVELS for n, _ in forms}
        launches = {}
        copies = {L: [] for L in LEVELS}
        encode = []
        assert torch.cuda.current_stream().cuda_stream == 0                  # torch's events are recorded on the null stream
        buf = {L: (torch.zeros(max(16, bytes_moved(w, h, L) // 2), dtype=torch.uint8, device="cuda"),
                   torch.zeros(max(16, bytes_moved(w, h, L) // 2), dtype=torch.uint8, device="cuda")) for L in LEVELS}
        with ds.glare(w, h) as g, ds.tone(w, h) as t:
            t.load_device(d_in)
            t.meter()
            # the two forms give the same bits on this frame
            for L in LEVELS:
                outs = []
                for n, form in forms:
                    g.set_form(form)
                    g.apply_device(d_in, d_out, levels=L)
                    launches[L, n] = g.info().last_launches
                    torch.cuda.synchronize()
                    outs.append(d_out.view(torch.int32).clone())
                assert torch.equal(outs[0], outs[1]), f"{key}: FUSED differs from PLAIN at L = {L}"
            for rep in range(repeats + 1):                                   # the first round is the warm-up
                for L in LEVELS:
                    for n, form in forms:
                        g.set_form(form)
                        p = g.params(levels=L)
                        took = batch_ms(torch, lambda: g.apply_device(d_in, d_out, params=p))
                        if rep:
                            ms[L, n].append(took)
                    src, dst = buf[L]
                    c = batch_ms(torch, lambda: dst.copy_(src))
                    if rep:
                        copies[L].append(c)
                tp = t.params()
                e = batch_ms(torch, lambda: t.encode_device(d_codes, params=tp))
                if rep:
                    encode.append(e)
        line = {"part": "timing", "case": key, "scene": name, "width": w, "height": h, "repeats": repeats, "batch": BATCH,
                "fused_equals_plain": True, "tone_encode_ms": spread(encode)}
        for L in LEVELS:
            for n, _ in forms:
                line[f"L{L}_{n}_ms"] = spread(ms[L, n])
                line[f"L{L}_{n}_ms_all"] = [round(x, 4) for x in ms[L, n]]
                line[f"L{L}_{n}_launches"] = launches[L, n]
            line[f"L{L}_bytes"] = bytes_moved(w, h, L)
            line[f"L{L}_copy_ms"] = spread(copies[L])
            line[f"L{L}_fused_over_plain"] = round(med(ms[L, "fused"]) / med(ms[L, "plain"]), 4)
        print(json.dumps(line), flush=True)
    finally:
        ds.close()
        hs.close()


def write_ppm(path, codes):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (codes.shape[1], codes.shape[0]))
        f.write(np.ascontiguousarray(codes, np.uint8).tobytes())


def lamp(out_dir):
    from film_report import setup
    torch, name, w, h, hs, cam, ds = setup("cornell")
    try:
        frame, _ = ds.render(cam, hs.params(w, 64, 50, seed=2, height=h))
        frame = np.ascontiguousarray(frame, np.float32).reshape(h, w, 3)
        with ds.glare(w, h) as g, ds.tone(w, h) as t:
            t.load(frame)
            info = t.meter()
            plain = t.encode(flags=0, exposure=info.exposure)             # the same exposure for both, alone
            spreaded = g.apply(frame)
            t.load(spreaded)
            glared = t.encode(flags=0, exposure=info.exposure)
            p = g.params()
        lum = frame.sum(axis=2)
        y, x = np.unravel_index(int(np.argmax(np.where(np.isfinite(lum), lum, -1.0))), lum.shape)
        row = h - 1 - int(y)                                                   # the codes' row 0 is the top
        x0, y0 = min(max(int(x) - 120, 0), w - 240), min(max(row - 80, 0), h - 160)
        crop = lambda c: c[y0:y0 + 160, x0:x0 + 240]
        write_ppm(os.path.join(out_dir, "lamp_plain.ppm"), crop(plain))
        write_ppm(os.path.join(out_dir, "lamp_glare.ppm"), crop(glared))
        a, b = crop(plain).astype(np.int64), crop(glared).astype(np.int64)
        white = lambda c: int((c.min(axis=2) == 255).sum())
        line = {"part": "lamp", "scene": name, "width": w, "height": h, "spp": 64, "levels": p.levels, "strength": round(p.strength, 4),
                "exposure": round(float(info.exposure), 5), "crop": [x0, y0, 240, 160], "frame_max": round(float(np.nanmax(frame)), 3),
                "clipped_pixels_plain": white(a), "clipped_pixels_glare": white(b),
                "crop_mean_code_plain": round(float(a.mean()), 3), "crop_mean_code_glare": round(float(b.mean()), 3),
                "codes_changed_in_crop": int((a != b).any(axis=2).sum()),
                "frame_sum_ratio": round(float(spreaded.astype(np.float64).sum() / frame.astype(np.float64).sum()), 9)}
        print(json.dumps(line), flush=True)
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="c2,cornell,final,lamp")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glare", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one step and print its lines")
    args = ap.parse_args()
    out_dir = os.path.dirname(os.path.abspath(args.out))
    if args.child:
        lamp(out_dir) if args.child == "lamp" else timing(args.child, args.repeats)
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
