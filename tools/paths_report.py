"""Path batches (vk_paths_*): the device-resident wavefront loop next to the host loop it replaces and next to vk_trace_radiance, and
the cost of its compaction.  Writes profiles/paths/report.jsonl (one JSON line per frame) and prints them.

    python tools/paths_report.py [--repeats 3] [--cases c2,cornell,final] [--out profiles/paths/report.jsonl]

Frames: those of tools/trace_rays_report.py — C2's scene 1920x1080, cornell_box 900x900, final_scene 800x800 — with the pixel-centre
primary rays, row-major, one path per ray, max_depth 50, the scene's own integrator and background.
After a warm-up of each, three loops run interleaved in one process, --repeats times, every value kept and the median reported:
  (a) DeviceScene.wavefront_radiance: vk_trace_rays and vk_shade_hits in turn, the survivors compacted in numpy (the host loop);
  (b) a path batch: PathBatch.begin, then step until nothing is live (the upload of rays and states is inside its wall time);
  (c) vk_trace_radiance at one sample a ray.
Wall seconds are time.perf_counter around the whole loop; kernel milliseconds are the calls' own (device events around the launches,
summed).  Then the batch runs once more per repeat one bounce a call, and per bounce vk_debug_paths_last_ms gives the trace, shade and
compaction milliseconds (events between the three parts).  The compaction reads 100 bytes an item (its vk_shaded and its id) and writes
84 per survivor (ray, state, id) or 52 per retired item (state, status); beside it stands a device-to-device copy of the same byte
count (n bytes moved = n / 2 in and n / 2 out), and beside trace_paths_kernel stands trace_rays_kernel (vk_trace_rays' kernel_ms) on the
same rays.  Nothing passes or fails.  Each frame is a timed step of its own: a child process under a time limit; after one fails no
further one is started."""
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
f32 = np.float32
med = statistics.median


def r4(xs):
    return [round(float(x), 4) for x in xs]


def frame(key, repeats):
    import torch            # first: its wheel carries its own HIP runtime, which must be the one that initialises the device
    torch.cuda.init()
    from shade_report import copy_ms
    from trace_rays_report import CASES, primary_rays
    from vecchio_amd import DeviceScene, HostScene
    from vecchio_amd.scene import make_path_states
    name, w, h = CASES[key]
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        rays = np.ascontiguousarray(primary_rays(cam, w, h).reshape(-1))
        n = len(rays)
        kw = dict(max_depth=50, integrator=hs.integrator, background=hs.background, background_color=hs.background_color)
        seed = 2
        states = make_path_states(n, seed, 0, 0)
        rkw = dict(kw, seed=seed, first_index=0, samples_per_ray=1)
        pb = ds.paths(n)

        def host_loop():
            t0 = time.perf_counter()
            res, bounces = ds.wavefront_radiance(rays, seed, 0, 0, return_bounces=True, **kw)
            return time.perf_counter() - t0, sum(b["trace"].kernel_ms + b["shade"].kernel_ms for b in bounces), res, len(bounces)

        def batch():
            t0 = time.perf_counter()
            pb.begin(rays, states, **kw)
            st = pb.step(1 << 20)
            return time.perf_counter() - t0, st.kernel_ms, st

        def query():
            t0 = time.perf_counter()
            _, st = ds.trace_radiance(rays, return_stats=True, **rkw)
            return time.perf_counter() - t0, st.kernel_ms

        _, _, res_a, n_bounces = host_loop(); _, _, st_b = batch(); query()        # warm-up
        res_b = pb.radiance()
        a, b, c = [], [], []
        for _ in range(repeats):                                                    # interleaved
            a.append(host_loop()[:2]); b.append(batch()[:2]); c.append(query())
        # without media the two loops are the same samples
        same = None if hs.desc.contents.n_media else bool(np.array_equal(res_a.view(np.uint32), res_b.view(np.uint32)))
        # one bounce a call: the three parts of every bounce, and trace_rays_kernel on the same rays
        per = []
        for rep in range(repeats):
            pb.begin(rays, states, **kw)
            k = 0
            while pb.info().live:
                live_rays = pb.read()[1] if rep == 0 else None
                st = pb.step(1)
                ms = pb.last_ms()
                if rep == 0:
                    _, ts = ds.trace_rays(live_rays, seed, 0, return_stats=True)      # warm-up of the shape
                    tr = []
                    for _ in range(repeats):
                        _, ts = ds.trace_rays(live_rays, seed, 0, return_stats=True)
                        tr.append(ts.kernel_ms)
                    m = int(st.live)
                    nbytes = 100 * int(st.traced) + 84 * m + 52 * (int(st.traced) - m)
                    per.append({"bounce": k + 1, "items": int(st.traced), "survivors": m, "compact_bytes": nbytes, "trace_paths": [], "shade": [],
                                "compact": [], "trace_rays_ms_all": r4(tr), "copy_ms_all": r4(copy_ms(torch, nbytes, repeats))})
                per[k]["trace_paths"].append(ms[0]); per[k]["shade"].append(ms[1]); per[k]["compact"].append(ms[2])
                k += 1
        bounces = []
        for p in per:
            qc, qcopy = med(p["compact"]), med(p["copy_ms_all"])
            bounces.append({"bounce": p["bounce"], "items": p["items"], "survivors": p["survivors"], "compact_bytes": p["compact_bytes"],
                            "compact_ms": round(qc, 4), "compact_ms_all": r4(p["compact"]),
                            "compact_gbytes_per_s": round(p["compact_bytes"] / qc / 1e6, 1),
                            "copy_ms": round(qcopy, 4), "copy_ms_all": p["copy_ms_all"],
                            "copy_gbytes_per_s": round(p["compact_bytes"] / qcopy / 1e6, 1), "compact_over_copy": round(qc / qcopy, 3),
                            "trace_paths_ms": round(med(p["trace_paths"]), 4), "trace_paths_ms_all": r4(p["trace_paths"]),
                            "trace_rays_ms": round(med(p["trace_rays_ms_all"]), 4), "trace_rays_ms_all": p["trace_rays_ms_all"],
                            "shade_ms": round(med(p["shade"]), 4), "shade_ms_all": r4(p["shade"])})
        wa, wb, wc = med(x[0] for x in a), med(x[0] for x in b), med(x[0] for x in c)
        ka, kb, kc = med(x[1] for x in a), med(x[1] for x in b), med(x[1] for x in c)
        print(json.dumps({"case": key, "scene": name, "width": w, "height": h, "rays": n, "repeats": repeats, "n_bounces": n_bounces,
                          "media": int(hs.desc.contents.n_media), "batch_equals_host_loop_bit_for_bit": same,
                          "host_loop_wall_s": round(wa, 4), "host_loop_wall_s_all": r4(x[0] for x in a),
                          "host_loop_kernel_ms": round(ka, 3), "host_loop_kernel_ms_all": r4(x[1] for x in a),
                          "batch_wall_s": round(wb, 4), "batch_wall_s_all": r4(x[0] for x in b),
                          "batch_kernel_ms": round(kb, 3), "batch_kernel_ms_all": r4(x[1] for x in b),
                          "radiance_wall_s": round(wc, 4), "radiance_wall_s_all": r4(x[0] for x in c),
                          "radiance_kernel_ms": round(kc, 3), "radiance_kernel_ms_all": r4(x[1] for x in c),
                          "batch_wall_over_host_loop": round(wb / wa, 4), "batch_wall_over_radiance": round(wb / wc, 4),
                          "batch_kernel_over_radiance": round(kb / kc, 4),
                          "compact_share_of_batch_kernel": round(sum(x["compact_ms"] for x in bounces) / kb, 4),
                          "batch_launches": int(st_b.kernel_launches), "bounces": bounces}), flush=True)
        pb.close()
    finally:
        ds.close()
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,cornell,final")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paths", "report.jsonl"))
    ap.add_argument("--child", default=None, help="(internal) run one case and print its line")
    args = ap.parse_args()
    if args.child:
        frame(args.child, args.repeats)
        return 0
    lines = []
    status = 0
    for key in args.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", key, "--repeats", str(args.repeats), "--out", args.out],
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
