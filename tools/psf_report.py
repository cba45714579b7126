"""Point-spread function (vk_psf_*): a load and one apply in both forms on whole frames, the LDS form's four passes each next to a device
copy of the bytes the pass must move, and, for scale, the default vk_glare apply and vk_tone_encode_device on the same frame; and the
Cornell box's lamp with and without the star.  Writes profiles/psf/report.jsonl (one JSON line per row) and prints them.

    python tools/psf_report.py [--repeats 9] [--steps c2,cornell,final,lamp] [--out profiles/psf/report.jsonl]

Timing (steps c2, cornell, final: C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800): the frame is rendered once at 4
samples per pixel and stays on the device; per K = 65, 257 and 513 a handle of that kmax with vk_psf_star(K, 6, 0, 8, 0.1) loaded.
Behind a warm-up round, --repeats rounds run interleaved — per round and K the load, the PLAIN apply, the LDS apply (whose four passes
come from the events the library records between them: vk_psf_debug_last_pass_ms), the four copies, then once per round the glare apply
and the encode —; every value is kept, the median and the spread (min, max) reported.  An apply here is a fraction of a millisecond to
tens of milliseconds, so a sample is ONE call between two events on the null stream (the stream every one of these calls runs on), in
device milliseconds; the load is host wall time around vk_psf_load (it validates and normalises on the host, uploads and waits).
Before the rounds each frame's LDS output is compared with its PLAIN output as floats at every K; a difference ends the step.

The bytes a pass of the LDS form must move, with P = Px * Py * 8 (a plane) and F = W * H * 12 (the frame): rows forward read F and write
3 * H * Px * 8 (the rows below H only); columns forward read those and write 3 P; the product and rows inverse read 3 P of F and 3 P of
G and write 3 P; columns inverse with the composite read 3 * Py * W * 8 (the columns left of W only) and F and write F.  The copy of as
many bytes (half read, half written) is the floor a pass is held against: pass_over_copy says how far from the bandwidth bound it is.

Step lamp: cornell_box at 900x900 and 64 samples per pixel through ACES and sRGB at the metered exposure of the frame without the star,
without and with the star (K = 257, six streaks, chroma 0.1, the library's default strength); a 240 x 160 crop around the brightest
pixel of each goes to lamp_plain.ppm and lamp_star.ppm beside the report.  Nothing passes or fails.  Each step is a child process under a
time limit; after one fails no further one is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_LIMIT_S = 240
KS = (65, 257, 513)
PASSES = ("rows_forward", "columns_forward", "product_rows_inverse", "columns_inverse_composite")
med = statistics.median


def spread(xs):
    return {"median": round(med(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def pass_bytes(W, H, K):
    Px, Py = pow2(W + K - 1), pow2(H + K - 1)
    P, F = Px * Py * 8, W * H * 12
    rows = 3 * H * Px * 8
    cols = 3 * Py * W * 8
    return [F + rows, rows + 3 * P, 9 * P, cols + 2 * F]


def event_ms(torch, call):
    """one call between two events on the null stream: device milliseconds"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timing(key, repeats):
    from film_report import setup
    torch, name, w, h, hs, cam, ds = setup(key)
    from vecchio_amd import ffi
    from vecchio_amd.scene import Psf
    try:
        frame, _ = ds.render(cam, hs.params(w, 4, 50, seed=2, height=h))
        d_in = torch.from_numpy(np.ascontiguousarray(frame, np.float32).reshape(h, w, 3)).cuda()
        d_out = torch.zeros_like(d_in)
        d_codes = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        assert torch.cuda.current_stream().cuda_stream == 0                  # torch's events are recorded on the null stream
        forms = (("plain", ffi.VK_PSF_FORM_PLAIN), ("lds", ffi.VK_PSF_FORM_LDS))
        line = {"part": "timing", "case": key, "scene": name, "width": w, "height": h, "repeats": repeats}
        glare_ms, encode_ms = [], []
        stars = {K: Psf.star(K, 6, 0.0, 8.0, 0.1, lib=ds._lib) for K in KS}
        handles = {K: ds.psf(w, h, K) for K in KS}
        try:
            ms = {(K, n): [] for K in KS for n, _ in forms}
            load = {K: [] for K in KS}
            passes = {K: [[] for _ in PASSES] for K in KS}
            copies = {K: [[] for _ in PASSES] for K in KS}
            launches = {}
            bufs = {}
            for K in KS:
                g = handles[K]
                g.load(stars[K])
                outs = []
                for n, form in forms:
                    g.apply_device(d_in, d_out, form=form)
                    launches[K, n] = g.info().last_launches
                    torch.cuda.synchronize()
                    outs.append(d_out.clone())
                same = (outs[0] == outs[1]) | (torch.isnan(outs[0]) & torch.isnan(outs[1]))
                assert bool(same.all()), f"{key}: LDS differs from PLAIN at K = {K}"
                half = max(pass_bytes(w, h, K)) // 2
                bufs[K] = (torch.zeros(half, dtype=torch.uint8, device="cuda"), torch.zeros(half, dtype=torch.uint8, device="cuda"))
            with ds.glare(w, h) as gl, ds.tone(w, h) as t:
                t.load_device(d_in)
                t.meter()
                for rep in range(repeats + 1):                               # the first round is the warm-up
                    for K in KS:
                        g = handles[K]
                        t0 = time.perf_counter()
                        g.load(stars[K])
                        took = (time.perf_counter() - t0) * 1e3
                        if rep:
                            load[K].append(took)
                        for n, form in forms:
                            p = g.params(form=form)
                            took = event_ms(torch, lambda: g.apply_device(d_in, d_out, params=p))
                            if rep:
                                ms[K, n].append(took)
                                if n == "lds":
                                    for i, v in enumerate(g.last_pass_ms()):
                                        passes[K][i].append(v)
                        src, dst = bufs[K]
                        for i, b in enumerate(pass_bytes(w, h, K)):
                            c = event_ms(torch, lambda: dst[:b // 2].copy_(src[:b // 2]))
                            if rep:
                                copies[K][i].append(c)
                    gp, tp = gl.params(), t.params()
                    a = event_ms(torch, lambda: gl.apply_device(d_in, d_out, params=gp))
                    e = event_ms(torch, lambda: t.encode_device(d_codes, params=tp))
                    if rep:
                        glare_ms.append(a)
                        encode_ms.append(e)
            line["lds_equals_plain"] = True
            line["glare_default_ms"], line["tone_encode_ms"] = spread(glare_ms), spread(encode_ms)
            for K in KS:
                info = handles[K].info()
                line[f"K{K}_padded"] = [info.Px, info.Py]
                line[f"K{K}_scratch_mb"] = round(info.scratch_bytes / 2 ** 20, 1)
                line[f"K{K}_load_ms"] = spread(load[K])
                for n, _ in forms:
                    line[f"K{K}_{n}_ms"] = spread(ms[K, n])
                    line[f"K{K}_{n}_ms_all"] = [round(x, 4) for x in ms[K, n]]
                    line[f"K{K}_{n}_launches"] = launches[K, n]
                line[f"K{K}_lds_over_plain"] = round(med(ms[K, "lds"]) / med(ms[K, "plain"]), 4)
                for i, pname in enumerate(PASSES):
                    line[f"K{K}_{pname}_ms"] = spread(passes[K][i])
                    line[f"K{K}_{pname}_bytes"] = pass_bytes(w, h, K)[i]
                    line[f"K{K}_{pname}_copy_ms"] = spread(copies[K][i])
                    line[f"K{K}_{pname}_over_copy"] = round(med(passes[K][i]) / med(copies[K][i]), 3)
        finally:
            for g in handles.values():
                g.close()
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
    from vecchio_amd.scene import Psf
    try:
        frame, _ = ds.render(cam, hs.params(w, 64, 50, seed=2, height=h))
        frame = np.ascontiguousarray(frame, np.float32).reshape(h, w, 3)
        K = 257
        with ds.psf(w, h, K) as g, ds.tone(w, h) as t:
            g.load(Psf.star(K, 6, 0.0, 8.0, 0.1, lib=ds._lib))
            t.load(frame)
            info = t.meter()
            plain = t.encode(flags=0, exposure=info.exposure)             # the same exposure for both, alone
            spreaded = g.apply(frame)
            t.load(spreaded)
            starred = t.encode(flags=0, exposure=info.exposure)
            p = g.params()
        lum = frame.sum(axis=2)
        y, x = np.unravel_index(int(np.argmax(np.where(np.isfinite(lum), lum, -1.0))), lum.shape)
        row = h - 1 - int(y)                                                   # the codes' row 0 is the top
        x0, y0 = min(max(int(x) - 120, 0), w - 240), min(max(row - 80, 0), h - 160)
        crop = lambda c: c[y0:y0 + 160, x0:x0 + 240]
        write_ppm(os.path.join(out_dir, "lamp_plain.ppm"), crop(plain))
        write_ppm(os.path.join(out_dir, "lamp_star.ppm"), crop(starred))
        a, b = crop(plain).astype(np.int64), crop(starred).astype(np.int64)
        white = lambda c: int((c.min(axis=2) == 255).sum())
        line = {"part": "lamp", "scene": name, "width": w, "height": h, "spp": 64, "K": K, "streaks": 6, "chroma": 0.1,
                "strength": round(p.strength, 4), "exposure": round(float(info.exposure), 5), "crop": [x0, y0, 240, 160],
                "frame_max": round(float(np.nanmax(frame)), 3), "clipped_pixels_plain": white(a), "clipped_pixels_star": white(b),
                "crop_mean_code_plain": round(float(a.mean()), 3), "crop_mean_code_star": round(float(b.mean()), 3),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psf", "report.jsonl"))
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
