"""Russian roulette on the device (vk_roulette_set): a frame of 8 samples per pixel through regenerating runs of a path batch of 2^21
slots, plain, with the rule on the device, and with the same rule from the host.  Writes profiles/roulette/report.jsonl (one JSON line per
frame) and prints them.

    python tools/roulette_report.py [--repeats 3] [--cases c2,cornell,final] [--spp 8] [--capacity 2097152] [--rule 2,0.1,0.8]
                                    [--out profiles/roulette/report.jsonl]

Frames: those of tools/regen_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 — at max_depth 50, the scene's own
integrator and background.  After a warm-up of each, three routes run interleaved in one process, --repeats times, every value kept:
  (a) Film.render_regen, plain;
  (b) Film.render_regen with the rule set on the batch: the compaction's count pass applies it, nothing crosses the bus;
  (c) Film.render_regen with the rule off and a cull callback: PathBatch.read, tests/roulette_ref.py rule() in numpy, Film.regen_cull —
      84 bytes down and 5 up per live path and bounce, a second compaction, one bounce a call.
Each route is Film.render_regen's own calls in its own order with the steps' infos kept (reading an info costs the call nothing); wall
seconds are taken around them, kernel milliseconds, bounces, launches and traced rays are the infos' sums — (c)'s kernel milliseconds do
not hold its cull's marking pass and second compaction, which no info reports.
What has to hold: (b) and (c) have equal traced rays, bounces and film sums — it is the same rule —, and (b)'s wall seconds are below
(c)'s on every frame in every repetition; the line says whether it did.  (b) against (a) in kernel milliseconds and traced rays is
recorded and nothing is asked of it.  Each frame is a timed step of its own: a child process under a time limit; after one fails no
further one is started."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))      # roulette_ref: the rule in numpy, route (c)'s

STEP_LIMIT_S = 400
ALL = 0xFFFFFFFF
med = statistics.median


def r4(xs):
    return [round(float(x), 4) for x in xs]


def run(film, batch, rule=None, cull=None):
    """Film.render_regen(batch, cull=cull, roulette=rule)'s calls (one run: the report's frames have fewer than 2^32 paths) with every
    step's info kept: (wall seconds, totals, the film's raw sums)"""
    p = film.params
    film.reset()
    tot = dict(kernel_ms=0.0, bounces=0, launches=0, traced=0, steps=0)
    t0 = time.perf_counter()
    batch.set_roulette(*(rule or (None,)))
    film.regen_begin(batch, 0, 0, p.width, p.height, 0, p.samples_per_pixel)
    while True:
        st = film.regen_step(batch, 1 if cull is not None else ALL)
        tot["kernel_ms"] += st.kernel_ms; tot["bounces"] += st.bounces; tot["launches"] += st.kernel_launches
        tot["traced"] += st.traced; tot["steps"] += 1
        if st.live == 0 and st.remaining == 0:
            break
        if cull is not None and st.live:
            cull(batch)
    film.resolve()
    wall = time.perf_counter() - t0
    tot["culled"] = int(batch.info().retired[4])
    return wall, tot, film.debug_sums().copy()


def frame(key, repeats, spp, capacity, rule):
    import torch            # first: its wheel carries its own HIP runtime, which must be the one that initialises the device
    torch.cuda.init()
    import numpy as np
    import roulette_ref
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
        moved = [0]

        def host_rule(batch):
            _, _, states = batch.read()
            keep, scale = roulette_ref.rule(states, *rule)
            film.regen_cull(batch, keep, scale)
            moved[0] += len(states) * 89

        routes = {"a": dict(), "b": dict(rule=rule), "c": dict(cull=host_rule)}
        for kw in routes.values():                                              # warm-up
            run(film, pb, **kw)
        got = {k: [] for k in routes}
        same_rule = True
        for _ in range(repeats):                                                # interleaved
            moved[0] = 0
            for k, kw in routes.items():
                got[k].append(run(film, pb, **kw))
            b, c = got["b"][-1], got["c"][-1]
            same_rule = same_rule and b[1]["traced"] == c[1]["traced"] and b[1]["bounces"] == c[1]["bounces"] and \
                b[1]["culled"] == c[1]["culled"] and bool(np.array_equal(b[2], c[2]))
        line = {"case": key, "scene": name, "width": w, "height": h, "samples_per_pixel": spp, "paths": w * h * spp, "capacity": capacity,
                "repeats": repeats, "rule_first_depth_q_min_q_max": list(rule)}
        for k in routes:
            line[f"{k}_wall_s_all"] = r4(x[0] for x in got[k])
            line[f"{k}_kernel_ms_all"] = r4(x[1]["kernel_ms"] for x in got[k])
            line[f"{k}_wall_s"] = round(med(x[0] for x in got[k]), 4)
            line[f"{k}_kernel_ms"] = round(med(x[1]["kernel_ms"] for x in got[k]), 3)
            for f in ("bounces", "launches", "traced", "steps", "culled"):
                line[f"{k}_{f}"] = got[k][0][1][f]
        line["c_bytes_over_the_bus_per_run"] = moved[0]
        line["b_and_c_equal_traced_bounces_culled_and_film_sums"] = same_rule
        line["b_wall_s_below_c_in_every_repeat"] = bool(all(y[0] < x[0] for x, y in zip(got["c"], got["b"])))
        line["b_wall_s_over_c"] = round(line["b_wall_s"] / line["c_wall_s"], 4)
        line["b_wall_s_over_a"] = round(line["b_wall_s"] / line["a_wall_s"], 4)
        line["b_kernel_ms_over_a"] = round(line["b_kernel_ms"] / line["a_kernel_ms"], 4)
        line["b_traced_over_a"] = round(line["b_traced"] / line["a_traced"], 4)
        line["what_has_to_hold_held"] = same_rule and line["b_wall_s_below_c_in_every_repeat"]
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
    ap.add_argument("--rule", default="2,0.1,0.8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roulette", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its line")
    args = ap.parse_args()
    fd, lo, hi = args.rule.split(",")
    rule = (int(fd), float(lo), float(hi))
    if args.child:
        frame(args.child, args.repeats, args.spp, args.capacity, rule)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats), "--spp", str(args.spp),
                                "--capacity", str(args.capacity), "--rule", args.rule, "--out", args.out], capture_output=True, text=True,
                               timeout=STEP_LIMIT_S)
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
