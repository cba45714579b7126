"""Regeneration (vk_regen_*): a frame of 8 samples per pixel through a path batch of 2^21 slots, by the window route and by a
regenerating run, next to vk_render.  Writes profiles/regen/report.jsonl (one JSON line per frame) and prints them.

    python tools/regen_report.py [--repeats 3] [--cases c2,cornell,final] [--spp 8] [--capacity 2097152] [--out profiles/regen/report.jsonl]

Frames: those of tools/paths_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 — at max_depth 50, the scene's own
integrator and background.  After a warm-up of each, three routes run interleaved in one process, --repeats times, every value kept:
  (a) the window route, Film.render: windows that fit the batch, each emitted, stepped to its end and deposited;
  (b) Film.render_regen: one regenerating run over the whole frame;
  (c) vk_render at the same sample count.
Wall seconds are those of the three calls as they are.  Kernel milliseconds, bounces, launches and the rays walked come from a second,
instrumented pass of (a) and (b) in the same repetition — the same calls in the same order, with the infos of the steps kept and, for
(a), the emit's and the deposit's events read after every window — so that reading them costs the timed call nothing.  (a)'s kernel
milliseconds are its steps' plus its emits' and deposits'; (b)'s are its steps', which hold the top-ups and the deposits.  Occupancy is
traced / (bounces * capacity).  The last bounce's four parts are vk_debug_regen_last_ms'.
What has to hold: (b) below (a) in kernel milliseconds and in wall seconds, on every frame in every repetition; the line says whether it
did.  (b) / (c) is recorded and nothing is asked of it.  Each frame is a timed step of its own: a child process under a time limit;
after one fails no further one is started."""
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


def window_route_instrumented(film, batch):
    """Film.render's windows and calls, with every step's info and every window's emit and deposit milliseconds kept"""
    p = film.params
    cap = int(batch.info().capacity)
    spp = p.samples_per_pixel
    ns = min(spp, cap)
    w = max(1, min(p.width, cap // ns))
    h = max(1, min(p.height, cap // (ns * w))) if w == p.width else 1
    tot = dict(kernel_ms=0.0, bounces=0, launches=0, traced=0, windows=0)
    for s0 in range(0, spp, ns):
        for y0 in range(0, p.height, h):
            for x0 in range(0, p.width, w):
                film.emit(batch, x0, y0, min(w, p.width - x0), min(h, p.height - y0), s0, min(ns, spp - s0))
                while True:
                    st = batch.step(1)
                    tot["kernel_ms"] += st.kernel_ms; tot["bounces"] += st.bounces; tot["launches"] += st.kernel_launches
                    tot["traced"] += st.traced
                    if not st.live:
                        break
                film.deposit(batch)
                ms = film.last_ms()
                tot["kernel_ms"] += ms[0] + ms[1]; tot["launches"] += 2; tot["windows"] += 1
    return tot, film.resolve()


def regen_instrumented(film, batch):
    """Film.render_regen's calls with the step's info kept (one run: the report's frames have fewer than 2^32 paths)"""
    p = film.params
    film.regen_begin(batch, 0, 0, p.width, p.height, 0, p.samples_per_pixel)
    st = film.regen_step(batch, 0xFFFFFFFF)
    assert st.live == 0 and st.remaining == 0
    tot = dict(kernel_ms=st.kernel_ms, bounces=st.bounces, launches=st.kernel_launches, traced=st.traced, last_ms=film.regen_last_ms(batch))
    return tot, film.resolve()


def frame(key, repeats, spp, capacity):
    import torch            # first: its wheel carries its own HIP runtime, which must be the one that initialises the device
    torch.cuda.init()
    from trace_rays_report import CASES
    from vecchio_amd import DeviceScene, HostScene
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        q = hs.params(w, spp, 50, seed=2, height=h)
        assert w * h * spp < 2 ** 32
        pb = ds.paths(capacity)
        film = ds.film(cam, q)
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

        def timed(call):
            film.reset()
            t0 = time.perf_counter()
            img = call()
            return time.perf_counter() - t0, img.copy()

        def render():
            t0 = time.perf_counter()
            img, st = ds.render(cam, q)
            return time.perf_counter() - t0, st.kernel_ms, img

        film.render(pb); film.reset(); film.render_regen(pb); render()          # warm-up
        a, b, c = [], [], []
        equal = {"a": True, "b": True, "a_instrumented": True, "b_instrumented": True}
        for _ in range(repeats):                                                # interleaved
            wa, ia = timed(lambda: film.render(pb))
            wb, ib = timed(lambda: film.render_regen(pb))
            wc, kc, ic = render()
            film.reset()
            ta, ia2 = window_route_instrumented(film, pb)
            ia2 = ia2.copy()
            film.reset()
            tb, ib2 = regen_instrumented(film, pb)
            for k, img in (("a", ia), ("b", ib), ("a_instrumented", ia2), ("b_instrumented", ib2)):
                equal[k] = equal[k] and bool(np.array_equal(bits(img), bits(ic)))
            a.append((wa, ta)); b.append((wb, tb)); c.append((wc, kc))
        inf = film.info()
        occ = lambda t: t["traced"] / (t["bounces"] * capacity)
        line = {"case": key, "scene": name, "width": w, "height": h, "samples_per_pixel": spp, "paths": w * h * spp, "capacity": capacity,
                "repeats": repeats,
                "frames_equal_bit_for_bit": {"a_and_c": equal["a"] and equal["a_instrumented"], "b_and_c": equal["b"] and equal["b_instrumented"]},
                "a_wall_s_all": r4(x[0] for x in a), "b_wall_s_all": r4(x[0] for x in b), "c_wall_s_all": r4(x[0] for x in c),
                "a_kernel_ms_all": r4(x[1]["kernel_ms"] for x in a), "b_kernel_ms_all": r4(x[1]["kernel_ms"] for x in b),
                "c_kernel_ms_all": r4(x[1] for x in c),
                "a_wall_s": round(med(x[0] for x in a), 4), "b_wall_s": round(med(x[0] for x in b), 4), "c_wall_s": round(med(x[0] for x in c), 4),
                "a_kernel_ms": round(med(x[1]["kernel_ms"] for x in a), 3), "b_kernel_ms": round(med(x[1]["kernel_ms"] for x in b), 3),
                "c_kernel_ms": round(med(x[1] for x in c), 3),
                "a_windows": a[0][1]["windows"], "a_bounces": a[0][1]["bounces"], "b_bounces": b[0][1]["bounces"],
                "a_launches": a[0][1]["launches"], "b_launches": b[0][1]["launches"],
                "a_traced": a[0][1]["traced"], "b_traced": b[0][1]["traced"],
                "a_mean_occupancy": round(occ(a[0][1]), 4), "b_mean_occupancy": round(occ(b[0][1]), 4),
                "b_last_bounce_ms_topup_trace_shade_compact_all": [r4(x[1]["last_ms"]) for x in b],
                "b_kernel_ms_below_a_in_every_repeat": bool(all(y[1]["kernel_ms"] < x[1]["kernel_ms"] for x, y in zip(a, b))),
                "b_wall_s_below_a_in_every_repeat": bool(all(y[0] < x[0] for x, y in zip(a, b))),
                "b_kernel_ms_over_a": round(med(x[1]["kernel_ms"] for x in b) / med(x[1]["kernel_ms"] for x in a), 4),
                "b_wall_s_over_a": round(med(x[0] for x in b) / med(x[0] for x in a), 4),
                "b_kernel_ms_over_c": round(med(x[1]["kernel_ms"] for x in b) / med(x[1] for x in c), 4),
                "b_wall_s_over_c": round(med(x[0] for x in b) / med(x[0] for x in c), 4),
                "deposited": int(inf.deposited), "dropped": int(inf.dropped), "clamped": int(inf.clamped)}
        line["what_has_to_hold_held"] = line["b_kernel_ms_below_a_in_every_repeat"] and line["b_wall_s_below_a_in_every_repeat"]
        print(json.dumps(line), flush=True)
        film.close(); pb.close()
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regen", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its line")
    args = ap.parse_args()
    if args.child:
        frame(args.child, args.repeats, args.spp, args.capacity)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats), "--spp", str(args.spp),
                                "--capacity", str(args.capacity), "--out", args.out], capture_output=True, text=True, timeout=STEP_LIMIT_S)
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
