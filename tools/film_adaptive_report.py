"""A film's adaptive regeneration (vk_adapt_*): a frame of up to 256 samples per pixel in 32-sample windows through a path batch of 2^21
slots, stopping the tiles whose error has converged, next to the adaptive vk_progress of the same decisions and to a non-adaptive
regenerating frame.  Writes profiles/film_adaptive/report.jsonl (one JSON line per frame) and prints them.

    python tools/film_adaptive_report.py [--repeats 3] [--cases c2,cornell,final] [--budget 256] [--window 32] [--capacity 2097152]

Frames: those of tools/regen_report.py — C2's scene 1920x1080, cornell_box 900x900 (partial tiles: the top-up searches the pixel prefix),
final_scene 800x800 — at max_depth 50.  The tolerance is tests/test_gpu_adaptive.py's recipe: the median over tiles of the largest
per-pixel standard error after half the budget, from a non-adaptive vk_progress handle.  After a warm-up, three routes run interleaved
in one process, --repeats times, every value kept, the median and the spread (max - min) reported:
  (a) Film.render_adaptive: per window a tile run (vk_adapt_begin, vk_regen_step) and vk_adapt_close;
  (b) the adaptive vk_progress handle with the same parameters, stepped until the budget is reached or no tile is active;
  (c) Film.render_regen at the whole budget, no tile ever stopping.
Wall seconds are those of the calls as they are; kernel milliseconds are the steps' (a, c: vk_regen_info, b: vk_stats).  Per window of
(a): the active tiles before it, the mean occupancy traced / (bounces * capacity), and the wall milliseconds of vk_adapt_close (it waits
for its record: launch, kernels and readback).  The tile top-up next to regen_emit_kernel: the first bounce of a tile run with every tile
active and of a rectangular run over the whole frame emit the same number of paths; both times are vk_debug_regen_last_ms[0], interleaved.
Nothing is asked of the numbers.  Each frame is a timed step of its own: a child process under a time limit; after one fails no further
one is started."""
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

STEP_LIMIT_S = 420
med = statistics.median


def r4(xs):
    return [round(float(x), 4) for x in xs]


def spread(xs):
    xs = list(xs)
    return round(float(max(xs) - min(xs)), 4)


def tolerance(ds, cam, q, window):
    """the median over tiles of the largest per-pixel standard error after half the budget"""
    with ds.progress(cam, q, stderr=True) as pr:
        for _ in range(max(2, q.samples_per_pixel // window // 2)):
            pr.step(window)
        se = pr.stderr().max(axis=2)
    h, w = se.shape
    tx, ty = (w + 7) // 8, (h + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), np.float32)
    pad[:h, :w] = se
    return float(np.median(pad.reshape(ty, 8, tx, 8).max(axis=(1, 3))))


def film_adaptive(film, batch, window, capacity, instrumented):
    """Film.render_adaptive's calls; instrumented: every step's info and every close's wall milliseconds kept"""
    spp = film.params.samples_per_pixel
    tot = dict(kernel_ms=0.0, windows=[])
    done, active = 0, film.tile_samples()[1].tiles_active
    while active and done < spp:
        n = min(window, spp - done)
        film.adapt_begin(batch, n)
        st = film.regen_step(batch, 0xFFFFFFFF)
        assert st.live == 0 and st.remaining == 0
        t0 = time.perf_counter()
        info = film.adapt_close(n)
        close_ms = (time.perf_counter() - t0) * 1e3
        if instrumented:
            tot["kernel_ms"] += st.kernel_ms
            tot["windows"].append(dict(tiles_active=int(active), bounces=int(st.bounces), kernel_ms=round(st.kernel_ms, 3),
                                       mean_occupancy=round(st.traced / (st.bounces * capacity), 4) if st.bounces else 0.0,
                                       close_wall_ms=round(close_ms, 4)))
        done, active = info.samples_done, info.tiles_active
    return tot, film.resolve_adaptive()


def progress_adaptive(ds, cam, q, ap, window):
    kernel_ms = 0.0
    with ds.progress(cam, q, adaptive=ap) as pr:
        done, img = 0, None
        while done < q.samples_per_pixel:
            img, st = pr.step(min(window, q.samples_per_pixel - done))
            kernel_ms += st.kernel_ms
            done = pr.info().samples_done
            if pr.tile_samples()[1].tiles_active == 0:
                break
        tmap, inf = pr.tile_samples()
    return kernel_ms, img.copy(), tmap, inf


def topup_pair(film, batch, p, window):
    """(tile top-up ms, regen_emit_kernel ms, paths) of the first bounce of a run over the whole frame, every tile active"""
    film.reset()
    film.adapt_begin(batch, window)
    st = film.regen_step(batch, 1)
    tile_ms, n = film.regen_last_ms(batch)[0], int(st.emitted)
    film.reset()
    film.regen_begin(batch, 0, 0, p.width, p.height, 0, window)
    st = film.regen_step(batch, 1)
    assert int(st.emitted) == n
    return tile_ms, film.regen_last_ms(batch)[0], n


def frame(key, repeats, budget, window, capacity):
    import torch            # first: its wheel carries its own HIP runtime, which must be the one that initialises the device
    torch.cuda.init()
    from trace_rays_report import CASES
    from vecchio_amd import DeviceScene, HostScene
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        q = hs.params(w, budget, 50, seed=2, height=h)
        assert w * h * budget < 2 ** 32                 # (c) is one run
        tol = tolerance(ds, cam, q, window)
        ap = dict(abs_tol=tol, rel_tol=0.0, min_samples=0, min_steps=2)
        pb = ds.paths(capacity)
        film = ds.film(cam, q)
        film.enable_adaptive(**ap)
        plain = ds.film(cam, q)
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

        def timed(call):
            t0 = time.perf_counter()
            out = call()
            return time.perf_counter() - t0, out

        film_adaptive(film, pb, window, capacity, False); progress_adaptive(ds, cam, q, ap, window)          # warm-up
        a, b, c, tops = [], [], [], []
        equal = True
        for _ in range(repeats):                                                # interleaved
            film.reset()
            wa, (_, ia) = timed(lambda: film_adaptive(film, pb, window, capacity, False))
            ia = ia.copy()
            wb, (kb, ib, tmap_b, inf_b) = timed(lambda: progress_adaptive(ds, cam, q, ap, window))
            plain.reset()
            plain.regen_begin(pb, 0, 0, w, h, 0, budget)
            wc, st = timed(lambda: plain.regen_step(pb, 0xFFFFFFFF))
            film.reset()
            ta, ia2 = film_adaptive(film, pb, window, capacity, True)
            tmap_a, inf_a = film.tile_samples()
            equal = equal and bool(np.array_equal(bits(ia), bits(ib)) and np.array_equal(bits(ia2), bits(ib)) and np.array_equal(tmap_a, tmap_b))
            a.append((wa, ta)); b.append((wb, kb)); c.append((wc, st.kernel_ms))
            tops.append(topup_pair(film, pb, q, window))
        line = {"case": key, "scene": name, "width": w, "height": h, "budget": budget, "window": window, "capacity": capacity,
                "repeats": repeats, "abs_tol": tol, "tiles_total": int(inf_a.tiles_total), "tiles_active_at_the_end": int(inf_a.tiles_active),
                "samples_rendered": int(inf_a.samples_rendered), "samples_of_the_whole_budget": w * h * budget,
                "film_and_progress_equal_bit_for_bit": equal,
                "a_wall_s_all": r4(x[0] for x in a), "b_wall_s_all": r4(x[0] for x in b), "c_wall_s_all": r4(x[0] for x in c),
                "a_kernel_ms_all": r4(x[1]["kernel_ms"] for x in a), "b_kernel_ms_all": r4(x[1] for x in b), "c_kernel_ms_all": r4(x[1] for x in c),
                "a_wall_s": round(med(x[0] for x in a), 4), "b_wall_s": round(med(x[0] for x in b), 4), "c_wall_s": round(med(x[0] for x in c), 4),
                "a_wall_s_spread": spread(x[0] for x in a), "b_wall_s_spread": spread(x[0] for x in b), "c_wall_s_spread": spread(x[0] for x in c),
                "a_kernel_ms": round(med(x[1]["kernel_ms"] for x in a), 3), "b_kernel_ms": round(med(x[1] for x in b), 3),
                "c_kernel_ms": round(med(x[1] for x in c), 3),
                "a_kernel_ms_spread": spread(x[1]["kernel_ms"] for x in a), "b_kernel_ms_spread": spread(x[1] for x in b),
                "c_kernel_ms_spread": spread(x[1] for x in c),
                "a_windows": a[0][1]["windows"],
                "a_close_wall_ms_median": round(med(x["close_wall_ms"] for r in a for x in r[1]["windows"]), 4),
                "topup_paths": tops[0][2], "tile_topup_ms_all": r4(x[0] for x in tops), "regen_emit_ms_all": r4(x[1] for x in tops),
                "tile_topup_ms": round(med(x[0] for x in tops), 4), "regen_emit_ms": round(med(x[1] for x in tops), 4),
                "tile_topup_ms_spread": spread(x[0] for x in tops), "regen_emit_ms_spread": spread(x[1] for x in tops)}
        line["tile_topup_slower_than_the_spread"] = bool(line["tile_topup_ms"] - line["regen_emit_ms"] >
                                                         max(line["tile_topup_ms_spread"], line["regen_emit_ms_spread"]))
        print(json.dumps(line), flush=True)
        film.close(); plain.close(); pb.close()
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "film_adaptive", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its line")
    args = ap.parse_args()
    if args.child:
        frame(args.child, args.repeats, args.budget, args.window, args.capacity)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats), "--budget",
                                str(args.budget), "--window", str(args.window), "--capacity", str(args.capacity), "--out", args.out],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"case {key} ran into its time limit of {STEP_LIMIT_S} s; nothing further is started", file=sys.stderr)
            status = 1
            break
        got = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
        lines += got
        print("\n".join(got), flush=True)
        if r.returncode != 0:
            print(f"case {key} ended with status {r.returncode}; nothing further is started\n{r.stderr[-2000:]}", file=sys.stderr)
            status = 1
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
