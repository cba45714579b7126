"""What the denoiser (vk_denoise) costs and what it buys, on the GPU.  One JSON line per case plus a table on stderr.

    python tools/denoise_report.py [--repeats 7] [--part throughput|quality|all] [--sweep]

Throughput: C2's scene at 1920x1080, cornell_box at 900x900, final_scene at 800x800.  Inputs: a 16-spp progressive frame in 4 windows, its
standard error, AOVs at 16 spp.  Per level the HIP-event time of the plain and of the staged form of the level kernel (vk_debug_denoise_form,
vk_debug_denoise_last_ms; 8 levels, so that every tap spacing is timed), alternating the two forms, median of --repeats after a warm-up of
each; the total of the default call (5 levels, the shipped choice of forms) and its ratio to one 16-spp progressive step of the frame.
Quality: cornell_box 256x256 and random_spheres_iow 256x144 at 4, 16 and 64 spp (4 windows, AOVs at the same spp): relative MSE
mean((x - t)^2 / (t^2 + 0.01)) of the noisy mean and of the denoised image against vk_render at 8192 spp with another seed, and their
ratio; plus the frame tests/test_gpu_denoise.py pins (cornell_box 128x128, 16 spp).  --sweep: the same ratios over a grid of parameters."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vecchio_amd import DeviceScene, HostScene, ffi  # noqa: E402

THROUGHPUT = {"c2": ("random_spheres_iow", 1920, 1080), "cornell": ("cornell_box", 900, 900), "final": ("final_scene", 800, 800)}
QUALITY = [("cornell_box", 256, 256), ("random_spheres_iow", 256, 144)]


def frame(hs, ds, cam, w, h, spp, seed=5, windows=4):
    p = hs.params(w, spp, 50, seed=seed, height=h)
    step_ms = []
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(windows):
            img, st = pr.step(spp // windows)
            step_ms.append(st.kernel_ms)
        se = pr.stderr()
    aov, _ = ds.render_aov(cam, p)
    return dict(color=img.copy(), stderr3=se, albedo=aov["albedo"], normal=aov["normal"], depth=aov["depth"]), step_ms


def denoise(ds, g, **over):
    h, w = g["color"].shape[:2]
    return ds.denoise(g["color"], g["stderr3"], g["albedo"], g["normal"], g["depth"], params=ds.denoise_params(w, h, **over))


def level_ms(ds):
    ms = (C.c_double * 9)()
    assert ds._lib.vk_debug_denoise_last_ms(ds._h, C.byref(ms)) == ffi.VK_OK
    return list(ms)


def rel_mse(img, truth):
    return float(np.mean((img.astype(np.float64) - truth) ** 2 / (truth.astype(np.float64) ** 2 + 1e-2)))


def throughput(args):
    rows = []
    for key in args.cases.split(","):
        name, w, h = THROUGHPUT[key]
        hs = HostScene(name, 1)
        cam = hs.next_camera()
        ds = DeviceScene(hs.desc)
        try:
            g, _ = frame(hs, ds, cam, w, h, 16)
            p16 = hs.params(w, 32, 50, seed=5, height=h)
            with ds.progress(cam, p16) as pr:                  # one 16-spp step, after a warm-up step
                pr.step(16)
                step16 = pr.step(16)[1].kernel_ms
            per = {ffi.VK_DENOISE_FORM_PLAIN: [], ffi.VK_DENOISE_FORM_STAGED: []}
            outs = {}
            for rep in range(args.repeats + 1):                # rep 0 = the warm-up of both forms
                for form in per:
                    ds._lib.vk_debug_denoise_form(ds._h, form)
                    outs[form] = denoise(ds, g, levels=8)[0]
                    if rep:
                        per[form].append(level_ms(ds))
            assert np.array_equal(outs[ffi.VK_DENOISE_FORM_PLAIN].view(np.uint32), outs[ffi.VK_DENOISE_FORM_STAGED].view(np.uint32))
            ds._lib.vk_debug_denoise_form(ds._h, ffi.VK_DENOISE_FORM_AUTO)
            denoise(ds, g)
            total = statistics.median(denoise(ds, g)[1].kernel_ms for _ in range(args.repeats))
            med = lambda form, k: round(statistics.median(r[k] for r in per[form]), 4)
            row = {"part": "throughput", "case": key, "scene": name, "width": w, "height": h, "prepare_ms": med(ffi.VK_DENOISE_FORM_PLAIN, 0),
                   "plain_ms_per_level": [med(ffi.VK_DENOISE_FORM_PLAIN, 1 + i) for i in range(8)],
                   "staged_ms_per_level": [med(ffi.VK_DENOISE_FORM_STAGED, 1 + i) for i in range(8)],
                   "default_total_ms": round(total, 4), "step16_kernel_ms": round(step16, 3), "ratio_to_step16": round(total / step16, 4),
                   "repeats": args.repeats}
            rows.append(row)
            print(json.dumps(row), flush=True)
        finally:
            ds.close()
            hs.close()
    print("\ncase      s:    1      2      4      8     16     32     64    128 | default total, 16-spp step, ratio", file=sys.stderr)
    for r in rows:
        for form in ("plain", "staged"):
            print(f"{r['case']:8s}{form:7s}" + "".join(f"{v:7.3f}" for v in r[form + "_ms_per_level"])
                  + (f" | {r['default_total_ms']:.3f} ms, {r['step16_kernel_ms']:.2f} ms, {r['ratio_to_step16']:.3f}" if form == "plain" else ""),
                  file=sys.stderr)


SWEEP = [dict()] + [dict(sigma_l=v) for v in (1.0, 2.0, 8.0, 16.0)] + [dict(sigma_z=v) for v in (0.5, 2.0, 4.0)] + \
    [dict(levels=v) for v in (3, 4, 6)] + [dict(normal_squarings=v) for v in (5, 9)]


def quality(args):
    cases = [(n, w, h, spp) for n, w, h in QUALITY for spp in (4, 16, 64)] + [("cornell_box", 128, 128, 16)]
    truths = {}
    for name, w, h, spp in cases:
        hs = HostScene(name, 1)
        cam = hs.next_camera()
        ds = DeviceScene(hs.desc)
        try:
            if (name, w, h) not in truths:
                truths[(name, w, h)] = ds.render(cam, hs.params(w, 8192, 50, seed=77, height=h))[0]
            truth = truths[(name, w, h)]
            g, _ = frame(hs, ds, cam, w, h, spp)
            noisy = rel_mse(g["color"], truth)
            for over in (SWEEP if args.sweep else [dict()]):
                clean = rel_mse(denoise(ds, g, **over)[0], truth)
                print(json.dumps({"part": "quality", "scene": name, "width": w, "height": h, "spp": spp, "params": over,
                                  "relmse_noisy": round(noisy, 6), "relmse_denoised": round(clean, 6), "ratio": round(clean / noisy, 4)}),
                      flush=True)
        finally:
            ds.close()
            hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("all", "throughput", "quality"))
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    if args.part in ("all", "throughput"):
        throughput(args)
    if args.part in ("all", "quality"):
        quality(args)


if __name__ == "__main__":
    main()
